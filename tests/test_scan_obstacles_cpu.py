"""The height scan on the articulated obstacles without a GPU (include/qa_tsc_scan_obstacles.h): the float64 reference
(tests/scan_obstacles_ref.py) against closed forms, the scenes' own promises, the binding, which launch the bookkeeping chooses, the config
field, the command line, the refusals, and the ABI record."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd import _capi
from tests import depth_obstacles_scenes as dsc
from tests import scan_obstacles_ref as ref
from tests import scan_obstacles_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the reference against closed forms
@pytest.mark.parametrize("yaw", dsc.SEESAW_YAWS)
@pytest.mark.parametrize("q", dsc.SEESAW_TILTS)
def test_reference_reads_the_planks_top_plane(yaw, q):
    root, desc, state = sc.plank_scene(yaw, q)
    want, inside, edge = sc.plank_closed_form(root, desc, state)
    got = ref.scan(root, sc.grid(), sc.flat_map(), desc, state, sc.BORDER, sc.HS, sc.VS)
    keep = edge >= ref.EDGE
    assert (~keep).mean() <= 0.01
    assert np.array_equal(got["mode"][keep] == 1, inside[keep]) and inside.sum() >= 40 and (~inside).sum() >= 20
    # (the closed form turns by the descriptor's angle, the reference multiplies by its fp32 cos / sin, a vector up to 2^-24 off unit length:
    # over the plank's 1.5 m that is 1e-7 m of lx)
    assert np.abs(got["height"] - want)[keep].max() < 1e-7
    assert (got["static"] == 0).all()
    assert want[inside].max() > 0.26 > want[inside].min()                                        # both sides of the pivot


@pytest.mark.parametrize("q", (0.05, -0.05))
def test_reference_lifts_a_box_under_a_bar_record_by_q(q):
    root, desc, state, hmap = sc.box_scene(q)
    q = float(state[1, 0])                                             # 0.05 as fp32 holds it
    want, stated, in_fp = sc.box_closed_form(root, q)
    got = ref.scan(root, sc.grid(), hmap, desc, state, sc.BORDER, sc.HS, sc.VS)
    assert stated.sum() >= 60 and (stated & in_fp).sum() >= 15
    assert np.abs(got["height"] - want)[stated].max() < 1e-12
    assert np.array_equal(got["mode"][stated] == 2, in_fp[stated])
    assert {round(float(v), 6) for v in want[stated]} == {0.0, round(q, 6), round(0.3 + q, 6)}   # ground, lifted ground, lifted box


def test_the_course_scenes_keep_their_promises():
    """what tests/test_scan_obstacles.py relies on, from the reference alone: robots turned away from yaw 0, see-saw robots with point 67 on
    the plank and with covered points in the four-lane tail, bar / tyre robots with covered rows, and fewer than 1 % of the points doubtful"""
    for kinds in (sc.MIXED, (sc.SEESAW,) * 9, (sc.BAR, sc.TYRE) * 4 + (sc.BAR,)):
        p, r = sc.placed(kinds), sc.reference(kinds)
        yaw = 2 * np.arctan2(p["root"][:, 5], p["root"][:, 6])
        assert (np.abs(np.sin(yaw)) > 0.05).all()
        for n in (1, 5, 9):
            assert r["doubtful"][:n].mean() <= 0.01, (kinds, n, r["doubtful"][:n].sum())
        for i, kind in enumerate(kinds):
            covered = (r["mode"][i] == (1 if kind == sc.SEESAW else 2)) & ~r["doubtful"][i]
            assert covered.sum() >= (30 if kind == sc.SEESAW else 10), (kinds, i, covered.sum())
            assert (r["mode"][i] == 0).sum() >= 20
    r = sc.reference((sc.SEESAW,) * 9)
    ok = ~r["doubtful"]
    assert (r["mode"][0, ref.CENTRE] == 1) and ok[0, ref.CENTRE]                                # env 0, alone in the N = 1 case, has point 67 on its plank
    assert ((r["mode"][:5, 128:] == 1) & ok[:5, 128:]).any() and (r["mode"][1, 128:] == 1).sum() >= 3
    assert (r["mode"][1, ref.CENTRE] == 0)                                                      # and another see-saw robot has it beside the plank
    hs = r["height"][r["mode"] == 1]
    assert hs.max() > 0.35 and hs.min() < 0.2                                                   # raised ends and lowered ones


# ------------------------------------------------------------------ library, binding
def test_library_exports_the_entry_point_and_the_binding_mirrors_the_header():
    import __graft_entry__ as g
    from quadrupedal_agility_amd import _cdecl
    from quadrupedal_agility_amd.tsc.legged_gym.task_level import QaTscScanObstacles
    g.build()
    lib = _capi.load_library()
    assert [h for h, n, _, _ in _cdecl.prototypes if n == "tsc_observations_obstacles"] == ["qa_tsc_scan_obstacles.h"]     # an extension: its own header
    assert "tsc_observations_obstacles" not in _capi.ABI_SYMBOLS
    f = lib.qa_tsc_observations_obstacles
    assert f.restype == C.c_int and len(f.argtypes) == 4
    assert f(None, None, None, None) == -1                              # QA_E_ARG (nothing touches the device)
    assert b"qa_tsc_observations_obstacles" in lib.qa_last_error()
    assert C.sizeof(QaTscScanObstacles) == 16
    assert [n for n, _ in QaTscScanObstacles._fields_] == ["obst_desc", "obst_state"]
    text = open(os.path.join(ROOT, "include", "qa_tsc_scan_obstacles.h")).read()
    assert "const float *obst_desc;" in text and "const float *obst_state;" in text and "int qa_tsc_observations_obstacles(" in text
    # qa_sim.h, the oracle's ABI, does not know the entry point
    assert "qa_tsc_observations_obstacles" not in open(os.path.join(ROOT, "include", "qa_sim.h")).read()


def test_abi_records_differ_from_the_one_before_by_additions_alone():
    """tests/golden/abi.json is the record as it was before this entry point; the entry point and its struct are recorded beside it, in
    tests/golden/abi_scan_obstacles.json.  The whole binding as tools/abi_dump.py sees it -- both records merged -- differs from abi.json by
    nothing but "only in one" lines for the new function and the new struct, and each record is what the library and the headers say now."""
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_dump
    old = json.load(open(abi_dump.GOLDEN))
    d, apart = abi_dump.dump(), abi_dump.dump_apart()
    assert abi_dump.differences(d, old) == []
    assert list(apart) == ["abi_scan_obstacles.json"]
    assert abi_dump.differences(apart["abi_scan_obstacles.json"], json.load(open(os.path.join(os.path.dirname(abi_dump.GOLDEN), "abi_scan_obstacles.json")))) == []
    new = abi_dump.merged(d, apart)
    assert abi_dump.differences(new, old) == ["/functions/tsc_observations_obstacles: only in one", "/structs/QaTscScanObstacles: only in one"]
    assert new["functions"]["tsc_observations_obstacles"] == {"list": "qa_tsc_scan_obstacles.h", "restype": "i32", "args": ["ptr"] * 4}
    assert new["structs"]["QaTscScanObstacles"] == old["structs"]["QaTscDepthObstacles"]              # the sibling's layout


# ------------------------------------------------------------------ bookkeeping, config, command line
class _Recorder:
    """an Api that notes the launches' names; the obstacle scan, which the oracle does not have, runs as the static one"""

    def __init__(self, api):
        self._api, self.prefix, self.names = api, api.prefix, []

    def launch(self, name, *args, on):
        self.names.append(name)
        if name == "tsc_observations_obstacles":
            name, args = "tsc_observations", args[:2]
        return self._api.launch(name, *args, on=on)

    def __getattr__(self, name):
        return getattr(self._api, name)


class _LibWithTheSymbol:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return (lambda *a: 0) if name == "qo_tsc_observations_obstacles" else getattr(self._lib, name)


def _observe(env):
    env.bk.compute_observations(env.root_states, env.dof_pos, env.dof_vel, env.action_history_buf, env.rigid_body_states, env.mass_params_tensor,
                                env.friction_coeffs_tensor, env.motor_strength)


def test_bookkeeping_launches_the_obstacle_scan_only_with_the_live_tensors():
    from tests.test_tsc_course_env import cpu_env
    env = cpu_env(4, seed=5)
    bk = env.bk
    assert bk._scan_obst is None
    rec = bk.api = _Recorder(bk.api)
    _observe(env)
    assert rec.names == ["tsc_observations"]
    args = (env.height_samples, env.height_points, env.default_dof_pos, env.default_dof_pos_all, env.key_body_ids.tolist())
    desc, state = env.sim.t["OBST_DESC"], env.obst_state
    with pytest.raises(NotImplementedError, match="qa_tsc_observations_obstacles"):            # the oracle has no twin of it
        bk.init_observations(*args, obst_desc=desc, obst_state=state)
    bk.lib = _LibWithTheSymbol(bk.lib)
    with pytest.raises(ValueError, match="go together"):
        bk.init_observations(*args, obst_desc=desc)
    for bad_desc, bad_state in ((desc[:, :2], state), (desc.double(), state), (desc, state.transpose(1, 2)), (desc, state[:3])):
        with pytest.raises(ValueError, match="contiguous float32"):
            bk.init_observations(*args, obst_desc=bad_desc, obst_state=bad_state)
    bk.init_observations(*args, obst_desc=desc, obst_state=state)
    assert bk._scan_obst[0] is desc and bk._scan_obst[1] is state                               # by reference: the live tensors
    del rec.names[:]
    _observe(env)
    assert rec.names == ["tsc_observations_obstacles"]
    bk.init_observations(*args)
    del rec.names[:]
    _observe(env)
    assert rec.names == ["tsc_observations"]


def test_config_field_and_command_line():
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    from quadrupedal_agility_amd.tsc.legged_gym.utils import helpers
    assert LeggedRobotCfg.obstacle.qa_scan_articulated is False and Go2AgilityCfg().obstacle.qa_scan_articulated is False
    assert helpers.get_args([]).scan_articulated is False
    env_cfg = Go2AgilityCfg()
    helpers.update_cfg_from_args(env_cfg, None, helpers.get_args(["--scan_articulated"]))
    assert env_cfg.obstacle.qa_scan_articulated is True and env_cfg.depth.qa_articulated is False
    env_cfg = Go2AgilityCfg()
    helpers.update_cfg_from_args(env_cfg, None, helpers.get_args(["--depth_articulated"]))
    assert env_cfg.obstacle.qa_scan_articulated is False


def test_the_flag_is_refused_where_it_cannot_work():
    from tests.test_tsc_course_env import cpu_env
    with pytest.raises(ValueError, match="obstacle.articulated"):
        cpu_env(4, seed=5, obstacle__qa_scan_articulated=True, obstacle__articulated=False)
    with pytest.raises(NotImplementedError, match="qa_tsc_observations_obstacles"):          # the oracle has no twin of it
        cpu_env(4, seed=5, obstacle__qa_scan_articulated=True)
    env = cpu_env(4, seed=5)                                                                  # off: nothing changes
    assert env.bk._scan_obst is None and isinstance(env.measured_heights, torch.Tensor)
