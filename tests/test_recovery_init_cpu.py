"""Recovery-pose resets and settable contact sets (include/qa_sim_reset.h) without a GPU: the host twin of tests/recovery_ref.py pinned to the
published Philox known answer and to the oracle's own reset stream, its pose mapping against THE REFERENCE'S outputs
(tests/golden/recovery_init.npz, tools/gen_golden_recovery.py), the per-step decision's statistics, the list -> mask translation and the
termination / collision restatement against the reference under six list pairs, the refusals, the symbols and the header.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi
from tests import recovery_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_TOL = dict(atol=2e-6, rtol=1e-5)                 # tests/test_mocap_reset.py's


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "recovery_init.npz"), allow_pickle=False)


def pairs(gold):
    return [([str(s) for s in gold[f"pair{i}_terminate_on"]], [str(s) for s in gold[f"pair{i}_penalize_on"]]) for i in range(int(gold["num_pairs"]))]


def edited_forces(gold):
    """CONTACT_FORCES of tests/golden/extra_rewards.npz's mid-step arena with the fixture's edits applied"""
    cf = np.load(os.path.join(ROOT, "tests", "golden", "extra_rewards.npz"), allow_pickle=False)["in_CONTACT_FORCES"].copy()
    quiet = gold["quiet_envs"]
    for lo, hi in ((0, 6), (7, 10), (11, 14), (15, 18)):
        cf[quiet, lo:hi] = 0.0
    cf[gold["edit_env"], gold["edit_body"]] = gold["edit_force"]
    return cf


# ---- the generator
def test_philox_known_answer():
    x = rr.philox4x32(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [f"{int(v):08x}" for v in x] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    y = rr.philox4x32(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]          # the second published vector
    assert [f"{int(v):08x}" for v in y] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_twin_reproduces_the_oracles_default_pose_reset():
    """ROOT_STATES[:, 7:13] after reset_all is u[12:18] - 0.5 of stream RS_RESET at the global env id: exact in fp32, so bit for bit"""
    from tests.oracle_lib import OracleSim, go2_cfg
    for seed, offset in ((1, 0), (23, 1000)):
        n = 16
        o = OracleSim(go2_cfg(n, seed=seed, env_id_offset=offset))
        o.global_step = 7
        o.reset_all()
        u = rr.rng4(seed, (np.arange(n) + offset)[:, None], 7, rr.RS_RESET, np.arange(5)[None, :]).reshape(n, 20)
        assert np.array_equal(o.t["ROOT_STATES"][:, 7:13], u[:, 12:18] - np.float32(0.5))
        assert (o.t["ROOT_STATES"][:, 7:13] != 0).all()


# ---- the mapping
def test_pose_restatement_equals_the_reference(gold):
    u = gold["reset_uniforms"]
    assert u.shape == (64, 33) and u.dtype == np.float32 and (np.abs(gold["reset_env_origins"]) > 1e-3).all()
    root, q, qd = rr.recovery_pose(u, gold["reset_default_dof_pos"], gold["reset_init_pos"], gold["reset_env_origins"])
    for name, got, want in (("root_states", root, gold["reset_root_states"]), ("dof_pos", q, gold["reset_dof_pos"]), ("dof_vel", qd, gold["reset_dof_vel"])):
        print(name, "max |twin - reference|", np.abs(got - want).max())
        assert np.allclose(got, want, **POSE_TOL), name
    # the draws reach every quadrant and calves past their stop (-2.7227 rad: default -1.8 x up to 2)
    assert (gold["reset_dof_pos"][:, 2::3] < -2.7227).any() and (gold["reset_root_states"][:, 6] < 0).any() and (gold["reset_root_states"][:, 6] > 0).any()


# ---- the decision
@pytest.mark.parametrize("seed", [1, 9, 23, 31])
def test_decision_share_is_the_probability(seed):
    u = rr.decision_uniform(seed, np.arange(10000))
    for p in (0.3, 0.5):
        share, sd = float((u < np.float32(p)).mean()), np.sqrt(p * (1 - p) / 10000)
        print("seed", seed, "p", p, "share", share, "deviation in sd", (share - p) / sd)
        assert abs(share - p) < 3 * sd
    assert not rr.recovery_steps(seed, np.arange(10000), 0.0).any() and rr.recovery_steps(seed, np.arange(10000), 1.0).all()
    assert (u >= 0).all() and (u < 1).all()


def test_decision_is_shared_and_both_branches_occur_early_at_seed_23():
    got = rr.recovery_steps(23, np.arange(12), 0.5).astype(int).tolist()
    assert got == [1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1]
    # the decision's counter holds no env id; the per-env draws do
    a, b = rr.recovery_uniforms(23, np.arange(4), 3), rr.recovery_uniforms(23, np.arange(4) + 1000, 3)
    assert not np.array_equal(a, b) and np.array_equal(rr.recovery_uniforms(23, [1001], 3)[0], b[1])


# ---- the masks
def test_list_to_mask_translation(gold):
    from quadrupedal_agility_amd.legged_gym.utils import cfg_to_c
    want = [(3, 12), (0, 0), (2, 13), (24, 2), (1, 20), (31, 31)]
    got = pairs(gold)
    assert got[0] == (["base", "hip"], ["thigh", "calf"]) and got[1] == ([], []) and got[2] == (["hip"], ["base", "thigh", "calf"]) and got[3] == (["calf", "foot"], ["hip"])
    for (term, pen), (tm, pm) in zip(got, want):
        assert (cfg_to_c.contact_class_mask(term), cfg_to_c.contact_class_mask(pen)) == (tm, pm) == (rr.class_mask(term), rr.class_mask(pen))
    assert (_capi.DEFAULT_TERMINATION_MASK, _capi.DEFAULT_PENALISED_MASK) == want[0] and rr.BITS == _capi.BODY_CLASS_BITS
    assert rr.BODY_NAMES == _capi.BODY_NAMES


def test_termination_and_collision_restatement_equals_the_reference(gold):
    cf = edited_forces(gold)
    epl = np.load(os.path.join(ROOT, "tests", "golden", "extra_rewards.npz"), allow_pickle=False)
    differs = 0
    for i, (term, pen) in enumerate(pairs(gold)):
        flag, count = rr.termination_and_collision(cf, rr.class_mask(term), rr.class_mask(pen))
        time_out = gold[f"pair{i}_time_out"]
        assert np.array_equal(flag | time_out, gold[f"pair{i}_reset"]), (term, pen)
        assert np.array_equal(count, gold[f"pair{i}_collision"]), (term, pen)
        assert np.array_equal(time_out, gold["pair0_time_out"]) and time_out.sum() >= 2
        differs += int((gold[f"pair{i}_reset"] != gold["pair0_reset"]).any()) + int((gold[f"pair{i}_collision"] != gold["pair0_collision"]).any())
    assert differs >= 8 and epl["in_EPISODE_LENGTH"].max() >= 1000          # the pairs tell apart; the time-outs are the arena's
    # the empty sets: only time-outs reset, nothing is counted
    assert np.array_equal(gold["pair1_reset"], gold["pair1_time_out"]) and (gold["pair1_collision"] == 0).all()


# ---- refusals
def test_config_translation_refuses_what_the_kernels_cannot_do():
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    from quadrupedal_agility_amd.legged_gym.utils import cfg_to_c

    class Engine:
        def __init__(self):
            self.calls = []
        def set_recovery_init(self, p):
            self.calls.append(("prob", p))
        def set_contact_sets(self, t, p):
            self.calls.append(("sets", t, p))
    for bad in (["Head"], ["Head_upper"], ["base", "Head_lower"], ["wheel"], ["FL_calf"], ["a"]):
        with pytest.raises(NotImplementedError):
            cfg_to_c.contact_class_mask(bad)
    cfg, e = Go2LocomotionCfg(), Engine()
    assert cfg_to_c.install_recovery_init(cfg, e) == 0.0 and cfg_to_c.install_contact_sets(cfg, e) == (3, 12) and e.calls == []      # as shipped: nothing is called
    assert cfg_to_c.install_contact_sets(cfg, object()) == (3, 12)
    for bad in (-0.1, 1.5, float("nan")):
        cfg.env.recovery_init_prob = bad
        with pytest.raises(ValueError, match="recovery_init_prob"):
            cfg_to_c.install_recovery_init(cfg, e)
    cfg.env.recovery_init_prob = 0.2
    cfg.asset.terminate_after_contacts_on = ["hip"]
    assert cfg_to_c.install_recovery_init(cfg, e) == 0.2 and cfg_to_c.install_contact_sets(cfg, e) == (2, 12)
    assert e.calls == [("prob", 0.2), ("sets", 2, 12)]
    with pytest.raises(NotImplementedError, match="qa_set_contact_sets"):
        cfg_to_c.install_contact_sets(cfg, object())
    with pytest.raises(NotImplementedError, match="qa_set_recovery_init"):
        cfg_to_c.install_recovery_init(cfg, object())


def test_probability_without_mocap_init_is_reported_and_left_off(capsys):
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    from quadrupedal_agility_amd.legged_gym.utils import cfg_to_c
    cfg = Go2LocomotionCfg()
    cfg.env.recovery_init_prob, cfg.env.mocap_state_init = 0.2, False
    assert cfg_to_c.install_recovery_init(cfg, object()) == 0.0
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "recovery_init_prob" in out and "mocap_state_init" in out


def test_train_flags_reach_the_config():
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    from quadrupedal_agility_amd.legged_gym.utils import helpers
    args = helpers.get_args(["--recovery_init_prob", "0.25", "--terminate_on", "hip", "--penalize_on", "base", "--penalize_on", "thigh"])
    cfg, _ = helpers.update_cfg_from_args(Go2LocomotionCfg(), None, args)
    assert cfg.env.recovery_init_prob == 0.25 and cfg.asset.terminate_after_contacts_on == ["hip"] and cfg.asset.penalize_contacts_on == ["base", "thigh"]
    cfg, _ = helpers.update_cfg_from_args(Go2LocomotionCfg(), None, helpers.get_args(["--terminate_on", "none", "--penalize_on", "none"]))
    assert cfg.asset.terminate_after_contacts_on == [] and cfg.asset.penalize_contacts_on == []          # the empty lists from the command line
    with pytest.raises(ValueError, match="stands alone"):
        helpers.update_cfg_from_args(Go2LocomotionCfg(), None, helpers.get_args(["--terminate_on", "none", "--terminate_on", "hip"]))
    cfg, _ = helpers.update_cfg_from_args(Go2LocomotionCfg(), None, helpers.get_args([]))
    assert cfg.env.recovery_init_prob == 0.0 and cfg.asset.terminate_after_contacts_on == ["base", "hip"] and cfg.asset.penalize_contacts_on == ["thigh", "calf"]


# ---- symbols and header
def test_library_exports_the_entry_points_and_capi_binds_them():
    import __graft_entry__ as g
    g.build()
    lib = _capi.load_library()
    for name in ("set_recovery_init", "set_contact_sets"):
        assert name in _capi.EXTENSION_SYMBOLS and name not in _capi.ABI_SYMBOLS
    f, s = lib.qa_set_recovery_init, lib.qa_set_contact_sets
    assert f.restype == C.c_int and f.argtypes == [C.c_void_p, C.c_float] and s.restype == C.c_int and s.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32]
    assert f(None, 0.5) == -1 and s(None, 3, 12) == -1                 # QA_E_ARG: no handle (nothing touches the device)
    text = open(os.path.join(ROOT, "include", "qa_sim_reset.h")).read()
    bits = {k[len("QA_BC_"):].lower(): int(v) for k, v in __import__("re").findall(r"^#define (QA_BC_[A-Z]+)\s+(\d+)u\s*$", text, __import__("re").M)}
    assert {k: bits[k] for k in _capi.BODY_CLASS_BITS} == _capi.BODY_CLASS_BITS and bits["all"] == 31


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "use_reset.c"
    src.write_text('#include "qa_sim_reset.h"\n'
                   "int use(qa_sim *s) { return qa_set_recovery_init(s, 0.2f) + qa_set_contact_sets(s, QA_BC_HIP, QA_BC_DEFAULT_PENALISED | QA_BC_BASE); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_reset.o")])
