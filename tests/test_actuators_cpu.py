"""CPU side of the actuator models (include/qa_sim_actuators.h): the gain resolver against the reference's loop, the make_actuators /
install_actuators contract in both trees, the library's entry point and its binding, the record of the ABI beside tests/golden/abi.json, and the
float64 restatement of the three laws (tests/actuators_ref.py) against hand-computed values."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi, _cdecl
from quadrupedal_agility_amd.legged_gym.utils import cfg_to_c
from tests import actuators_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bbc_cfg():
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = 8; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
    return cfg


def _tsc_cfg():
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    return Go2AgilityCfg()


def reference_loop(stiffness, damping, control_type):
    """bbc/legged_gym/envs/base/legged_robot.py:844-858, restated: (p_gains, d_gains, printed lines)"""
    p, d, lines = [0.0] * 12, [0.0] * 12, []
    for i, name in enumerate(_capi.DOF_NAMES):
        found = False
        for dof_name in stiffness.keys():
            if dof_name in name:
                p[i] = stiffness[dof_name]
                d[i] = damping[dof_name]
                found = True
        if not found:
            p[i] = 0.
            d[i] = 0.
            if control_type in ["P", "V"]:
                lines.append(f"PD gain of joint {name} were not defined, setting them to zero")
    return p, d, lines


DICTS = [({"joint": 40}, {"joint": 1.0}),
         ({"hip": 30, "thigh": 20, "calf": 25}, {"hip": 0.5, "thigh": 1.0, "calf": 0.75}),
         ({"joint": 20, "calf": 40}, {"joint": 0.5, "calf": 2.0}),                   # the later key overwrites the earlier one on the calves
         ({"hip": 30, "thigh": 20}, {"hip": 0.5, "thigh": 1.0})]                     # the calves stay unmatched


@pytest.mark.parametrize("stiffness,damping", DICTS)
@pytest.mark.parametrize("control_type", ["P", "V", "T"])
def test_resolver_is_the_references_loop(stiffness, damping, control_type, capsys):
    cfg = _bbc_cfg()
    cfg.control.stiffness, cfg.control.damping, cfg.control.control_type = stiffness, damping, control_type
    kp, kd = cfg_to_c.resolve_pd_gains(cfg)
    out = capsys.readouterr().out.splitlines()
    p, d, lines = reference_loop(stiffness, damping, control_type)
    assert kp == [float(v) for v in p] and kd == [float(v) for v in d] and out == lines
    if "calf" not in stiffness and "joint" not in stiffness:
        calves = [i for i, n in enumerate(_capi.DOF_NAMES) if "calf" in n]
        assert all(kp[i] == 0 and kd[i] == 0 for i in calves) and len(lines) == (4 if control_type != "T" else 0)
    if stiffness == {"joint": 20, "calf": 40}:
        assert kp == [20.0, 20.0, 40.0] * 4 and kd == [0.5, 0.5, 2.0] * 4


@pytest.mark.parametrize("make", [_bbc_cfg, _tsc_cfg])
def test_make_actuators_contract(make):
    cfg = make()
    assert cfg_to_c.make_actuators(cfg) is None                        # the Go2 defaults: P, one gain pair -- the step as it always ran
    assert cfg_to_c.config_gains(cfg) == (40.0, float(cfg.control.damping["joint"]))
    for ct in ("V", "T"):
        cfg = make(); cfg.control.control_type = ct
        a = cfg_to_c.make_actuators(cfg)
        assert a.control_type == ct and a.kp == [40.0] * 12 and a.kd == [float(cfg.control.damping["joint"])] * 12
    cfg = make(); cfg.control.stiffness = {"hip": 30, "thigh": 40, "calf": 50}; cfg.control.damping = {"hip": 1, "thigh": 1, "calf": 1}
    a = cfg_to_c.make_actuators(cfg)
    assert a.control_type == "P" and a.kp == [30.0, 40.0, 50.0] * 4 and a.kd == [1.0] * 12      # equal damping alone does not make it the default
    cfg = make(); cfg.control.control_type = "X"
    with pytest.raises(NameError, match="Unknown controller type: X"):
        cfg_to_c.make_actuators(cfg)
    for flag in ("qa_self_collision_hips", "qa_self_collision_thighs"):
        cfg = make(); cfg.control.control_type = "T"; setattr(cfg.asset, flag, True)
        with pytest.raises(ValueError) as e:
            cfg_to_c.make_actuators(cfg)
        assert "qa_set_actuators" in str(e.value) and "qa_self_collision_hips" in str(e.value) and "qa_self_collision_thighs" in str(e.value)
        cfg.control.control_type = "P"
        assert cfg_to_c.make_actuators(cfg) is None                    # the default model goes with every self-collision level


class _Recorder:
    def __init__(self):
        self.calls = []

    def set_actuators(self, a):
        self.calls.append(a)


@pytest.mark.parametrize("make", [_bbc_cfg, _tsc_cfg])
def test_install_actuators(make):
    cfg, r = make(), _Recorder()
    assert cfg_to_c.install_actuators(cfg, r) is None and r.calls == []            # the setter is never called for the default
    assert cfg_to_c.install_actuators(cfg, object()) is None                       # ... so any backend serves it
    cfg.control.control_type = "V"
    a = cfg_to_c.install_actuators(cfg, r)
    assert r.calls == [a] and a.control_type == "V"
    with pytest.raises(NotImplementedError, match="qa_set_actuators"):
        cfg_to_c.install_actuators(cfg, object())


def test_command_line_flags_set_the_control_node():
    from quadrupedal_agility_amd.legged_gym.utils import helpers
    cfg, _ = helpers.update_cfg_from_args(_bbc_cfg(), None, helpers.get_args([]))
    assert cfg.control.control_type == "P" and cfg.control.stiffness == {"joint": 40.0} and cfg_to_c.make_actuators(cfg) is None
    args = helpers.get_args(["--control_type", "V", "--pd_gains", "hip=30:0.8", "--pd_gains", "thigh=40:1", "--pd_gains", "calf=50:1.2"])
    cfg, _ = helpers.update_cfg_from_args(_bbc_cfg(), None, args)
    assert cfg.control.control_type == "V" and cfg.control.stiffness == {"hip": 30.0, "thigh": 40.0, "calf": 50.0}
    assert cfg.control.damping == {"hip": 0.8, "thigh": 1.0, "calf": 1.2}
    a = cfg_to_c.make_actuators(cfg)
    assert a.control_type == "V" and a.kp == [30.0, 40.0, 50.0] * 4 and a.kd == [0.8, 1.0, 1.2] * 4
    for bad in ("hip=30", "hip:30", "=30:1", "hip=a:b"):
        with pytest.raises(ValueError, match="--pd_gains"):
            helpers.update_cfg_from_args(_bbc_cfg(), None, helpers.get_args(["--pd_gains", bad]))


def test_both_envs_refuse_a_backend_without_the_setter_and_keep_the_default():
    from quadrupedal_agility_amd.legged_gym.envs.base import legged_robot as bbc
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as tsc
    from tests.oracle_backend import OracleBackend
    from tests.oracle_lib import load_oracle
    cfg = _bbc_cfg()
    env = bbc.LeggedRobot(cfg, sim_device="cpu", backend=OracleBackend)
    assert env.actuators is None and env.p_gains.shape == (12,) and env.d_gains.shape == (12,)
    assert env.p_gains.tolist() == [40.0] * 12 and env.d_gains.tolist() == [float(cfg.control.damping["joint"])] * 12
    cfg = _bbc_cfg(); cfg.control.control_type = "T"
    with pytest.raises(NotImplementedError, match="qa_set_actuators"):
        bbc.LeggedRobot(cfg, sim_device="cpu", backend=OracleBackend)
    kw = dict(sim_device="cpu", bookkeeping_lib=(load_oracle(), "qo_"))
    cfg = _tsc_cfg(); cfg.env.num_envs = 4
    env = tsc.LeggedRobot(cfg, backend=OracleBackend, **kw)
    assert env.actuators is None and env.p_gains.tolist() == [40.0] * 12 and env.d_gains.shape == (12,)
    cfg = _tsc_cfg(); cfg.env.num_envs = 4; cfg.control.stiffness = {"hip": 30, "thigh": 40, "calf": 50}; cfg.control.damping = {"hip": 1, "thigh": 1, "calf": 1}
    with pytest.raises(NotImplementedError, match="qa_set_actuators"):
        tsc.LeggedRobot(cfg, backend=OracleBackend, **kw)


def test_library_exports_the_entry_point_and_capi_binds_it():
    import __graft_entry__ as g
    g.build()
    assert ("qa_sim_actuators.hip", g._ENV_FLAGS) in g.HIP_SOURCES
    assert os.path.join(ROOT, "include", "qa_sim_actuators.h") in g._lib_sources()
    lib = _capi.load_library()
    assert "set_actuators" in _capi.EXTENSION_SYMBOLS and "set_actuators" not in _capi.ABI_SYMBOLS
    assert [h for h, n, _, _ in _cdecl.prototypes if n == "set_actuators"] == ["qa_sim_actuators.h"]
    f = lib.qa_set_actuators
    assert f.restype == C.c_int and len(f.argtypes) == 2
    assert f(None, None) == -1                                           # QA_E_ARG: no handle (nothing touches the device)
    s = _cdecl.struct("qa_actuators")
    assert C.sizeof(s) == 4 + 4 * 12 + 4 * 12 and [n for n, _ in s._fields_] == ["control_type", "kp", "kd"]
    assert f(None, C.byref(s())) == -1
    assert (_cdecl.consts["QA_ACTUATOR_P"], _cdecl.consts["QA_ACTUATOR_V"], _cdecl.consts["QA_ACTUATOR_T"]) == (0, 1, 2)
    text = open(os.path.join(ROOT, "include", "qa_sim_actuators.h")).read()
    assert "int qa_set_actuators(qa_sim *sim, const qa_actuators *actuators);" in text and "BEFORE the first recording" in text


def test_abi_record_apart_matches_and_abi_json_is_untouched():
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_dump
    old = json.load(open(abi_dump.GOLDEN))
    d = abi_dump.dump()
    assert abi_dump.differences(d, old) == []                            # tests/golden/abi.json is the record as it was
    assert "set_actuators" not in old["functions"] and "QaActuators" not in old["structs"]
    apart = abi_dump.dump_apart(_capi._RECORDED_APART_ENGINE)
    assert list(apart) == ["abi_actuators.json"]
    rec = json.load(open(os.path.join(os.path.dirname(abi_dump.GOLDEN), "abi_actuators.json")))
    assert abi_dump.differences(apart["abi_actuators.json"], rec) == []
    assert rec["functions"] == {"set_actuators": {"list": "qa_sim_actuators.h", "restype": "i32", "args": ["ptr", "ptr"]}}
    assert rec["structs"]["QaActuators"]["size"] == 100
    new = abi_dump.merged(d, apart)
    assert abi_dump.differences(new, old) == ["/functions/set_actuators: only in one", "/structs/QaActuators: only in one"]


def test_float64_laws_against_hand_computed_values():
    """one env, numbers small enough to check by hand (binary fractions: every value below is exact)"""
    act = np.zeros((1, 12)); act[0, 0] = 2.0; act[0, 1] = 2.0; act[0, 2] = -1.0
    q = np.full((1, 12), 0.5); qd = np.full((1, 12), 0.25); last = np.zeros((1, 12)); last[0, 1] = 0.125
    q0 = np.full(12, 1.0)
    kp = np.array([32.0, 16.0, 8.0] * 4); kd = np.array([2.0, 1.0, 0.5] * 4)
    kw = dict(q0=q0, action_scale=0.25, hip_scale_reduction=0.5, sim_dt=0.5)
    # scaled actions: joint 0 is a hip: 2 * 0.25 * 0.5 = 0.25; joint 1: 0.5; joint 2: -0.25
    assert ref.scaled_actions(act, 0.25, 0.5)[0, :3].tolist() == [0.25, 0.5, -0.25]
    tau, big = ref.torques("T", act, q, qd, last, kp, kd, **kw)
    assert tau[0, :4].tolist() == [0.25, 0.5, -0.25, 0.0] and big[0, :3].tolist() == [0.25, 0.5, 0.25]
    tau, big = ref.torques("P", act, q, qd, last, kp, kd, **kw)
    # joint 0: 32 * (0.25 + 1 - 0.5) - 2 * 0.25 = 24 - 0.5; joint 1: 16 * (0.5 + 1 - 0.5) - 0.25 = 15.75; joint 2: 8 * (-0.25 + 0.5) - 0.125 = 1.875
    assert tau[0, :3].tolist() == [23.5, 15.75, 1.875] and big[0, :3].tolist() == [32.0, 16.0, 8.0]
    strength = np.ones((2, 1, 12)); strength[0, 0, 0] = 0.5; strength[1, 0, 0] = 2.0
    tau, big = ref.torques("P", act, q, qd, last, kp, kd, strength=strength, **kw)
    assert tau[0, :2].tolist() == [16 * 0.75 - 4 * 0.25, 15.75] and big[0, 0] == 16.0
    tau, big = ref.torques("V", act, q, qd, last, kp, kd, **kw)
    # joint 0: 32 * (0.25 - 0.25) - 2 * (0.25 - 0) / 0.5 = -1; joint 1: 16 * (0.5 - 0.25) - 1 * (0.25 - 0.125) / 0.5 = 4 - 0.25; joint 2: 8 * (-0.5) - 0.5 * 0.25 / 0.5 = -4.25
    assert tau[0, :3].tolist() == [-1.0, 3.75, -4.25] and big[0, :3].tolist() == [1.0, 4.0, 4.25]
    tau_s, _ = ref.torques("V", act, q, qd, last, kp, kd, strength=strength, **kw)
    assert np.array_equal(tau, tau_s)                                    # the reference ignores the motor strength outside the P law
    assert ref.clamp(np.array([[23.5, -30.0, 1.0]]), np.array([20.0, 25.0, 40.0])).tolist() == [[20.0, -25.0, 1.0]]
    assert ref.clip_actions(np.array([[500.0, -3.0]]), 100.0, 0.25).tolist() == [[400.0, -3.0]]
    assert [c.tolist()[:1] for c in ref.state_coefficients("V", kp, kd, 0.5)] == [[0.0], [36.0]]
    assert [c.tolist()[:1] for c in ref.state_coefficients("P", kp, kd, 0.5)] == [[32.0], [2.0]]
    assert [c.tolist()[:1] for c in ref.state_coefficients("T", kp, kd, 0.5)] == [[0.0], [0.0]]
    with pytest.raises(NameError):
        ref.torques("X", act, q, qd, last, kp, kd, **kw)
