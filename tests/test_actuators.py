"""-m gpu: the actuator models of include/qa_sim_actuators.h in the fused env step (qa_set_actuators): the P law with per-joint gains against the
oracle's whole env step, the T and V laws against the oracle's simulate driven by the float64 laws of tests/actuators_ref.py, the routing
of the launches, and both env classes.

The oracle has no V or T law and one gain pair.  It serves all the same:
  P, per-joint gains   the oracle's motor strength IS a per-joint factor on kp / kd: with strength s_j / r_j from {0.5, 1, 2} the oracle computes
                       (s kp) err - (r kd) qd, the kernel with gains kp s_j, kd r_j the same products, exactly (powers of two).
  T and V              `decimation` calls of OracleSim.simulate(tau_k), tau_k from the float64 law on the oracle's own state, clamped, as fp32.
Both sides start from the same arena.  Sizes: 1, 64 (fills its workgroups) and 67 envs (one workgroup partly filled)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from quadrupedal_agility_amd import go2_limits
from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import Actuators
from tests import actuators_ref as ref
from tests.oracle_lib import OracleSim, go2_cfg
from tests.parity_tol import BUDGET, MEDIAN_TOL, TOL, check_flips, env_errors, env_mismatch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIMITS = np.asarray(go2_limits.TORQUE_LIMITS, np.float64)
OVER = dict(push_robots=0, add_noise=0)
FACTORS = np.array([0.5, 1.0, 2.0])


def pair(n, hf, seed, **over):
    """(q, oracle) on the plane or on the rough height field of tests/test_hip_parity.py, after the oracle's reset and three steps of motion"""
    from tests.test_hip_parity import make_terrain_pair
    if hf:
        q, o, _ = make_terrain_pair(n, seed, with_hip=False, **over)
    else:
        q = go2_cfg(n, seed=seed, **over); o = OracleSim(q)
    o.reset_all()
    o.t["EPISODE_LENGTH"][:] = 5
    rng = np.random.default_rng(seed)
    for _ in range(3):
        o.step(rng.normal(0, 0.5, (n, 12)).astype(np.float32))
    return q, o, rng


def handle(q, o, actuators=None):
    from quadrupedal_agility_amd.sim import QaSim
    h = QaSim(q, "cuda:0")
    if actuators is not None:
        h.set_actuators(actuators)
    h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
    return h


def actions_for(rng, n, big=8.0):
    """test_single_step_parity's actions; every fourth env gets saturating ones (8x there; `big` where the law needs more to reach the effort
    limits), so that the action clip and the effort clamp run"""
    act = rng.normal(0, 1.0, (n, 12)).astype(np.float32)
    act[::4] *= big
    return act


# ------------------------------------------------------------------ 1. P with per-joint gains, against the oracle's whole env step
def run_p(hf, n, fold):
    """fold "gains": the kernel runs without randomize_motor and carries s_j, r_j in its gains.  "strength_times_gains": both sides randomize the
    motor; the kernel's strength is s_j / u_j and its gains carry u_j -- the strength-times-gain product of the law.  Left out by construction:
    MOTOR_STRENGTH and its 24 entries of the privileged block of OBS (66:90), which state the strength itself."""
    qo, o, rng = pair(n, hf, 21 + n, randomize_motor=1, **OVER)
    s, r = rng.choice(FACTORS, 12), rng.choice(FACTORS, 12)
    o.t["MOTOR_STRENGTH"][0] = s; o.t["MOTOR_STRENGTH"][1] = r
    kp, kd = float(qo.kp), float(qo.kd)
    if fold == "gains":
        qh = type(qo).from_buffer_copy(qo); qh.randomize_motor = 0
        u_p, u_d, hs, hr = s, r, None, None
    else:
        qh = qo
        u_p, u_d = rng.choice(FACTORS, 12), rng.choice(FACTORS, 12)
        hs, hr = s / u_p, r / u_d                                      # exact: powers of two
    h = handle(qh, o, Actuators("P", kp * u_p, kd * u_d))
    flips, total, per_env = 0, 0, {k: [] for k in MEDIAN_TOL}
    for k in range(10):
        h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
        if hs is not None:
            h.t["MOTOR_STRENGTH"][0] = torch.from_numpy(np.broadcast_to(hs, (n, 12)).astype(np.float32)).cuda()
            h.t["MOTOR_STRENGTH"][1] = torch.from_numpy(np.broadcast_to(hr, (n, 12)).astype(np.float32)).cuda()
        act = rng.normal(0, 1.0, (n, 12)).astype(np.float32)
        if k % 7 == 3:
            act *= 8.0
        o.step(act); h.step(torch.from_numpy(act).cuda()); torch.cuda.synchronize()
        bad = np.zeros(n, bool)
        for name in TOL:
            got, exp = h.t[name].cpu().numpy(), o.t[name]
            if name == "OBS":
                got, exp = np.delete(got, np.s_[66:90], axis=1), np.delete(exp, np.s_[66:90], axis=1)
            bad |= env_mismatch(name, got, exp, n)
            if name in per_env:
                per_env[name].append(env_errors(name, got, exp, n))
        flips += int(bad.sum()); total += n
    med = {k: float(np.median(np.concatenate(v))) for k, v in per_env.items()}
    print("median env-step error per tensor:", {k: f"{v:.2e}" for k, v in med.items()})
    check_flips(f"actuators_P_{fold}_T{hf}_N{n}", flips, total, BUDGET["height_field" if hf else "plane"])
    assert not {k: v for k, v in med.items() if v > MEDIAN_TOL[k]}, med


@pytest.mark.parametrize("hf,n", [(0, 1), (0, 64), (0, 67), (1, 67)])
@pytest.mark.parametrize("fold", ["gains", "strength_times_gains"])
def test_p_law_with_per_joint_gains_is_the_oracles_step(hf, n, fold):
    run_p(hf, n, fold)


# ------------------------------------------------------------------ 2. T and V, physics against the oracle's simulate
def run_tv(hf, n, mode, seed=5):
    """one arena; the HIP side takes one step in mode T, then one in mode V (`mode` 0: the fused step, 1: physics_step); the reference
    trajectory is `decimation` oracle substeps under the float64 law.  Returns (env-steps outside the bounds, env-steps judged)."""
    q, o, rng = pair(n, hf, seed + n, randomize_motor=1, **OVER)           # the motor strength is drawn and must be ignored
    # velocity gains: a few N m per rad/s, and kd / sim_dt of 2, 1 and 4 -- the torques stay inside the effort limits except on the saturating envs
    kp = np.array([4.0, 3.0, 5.0] * 4); kd = np.array([0.01, 0.005, 0.02] * 4)
    q0 = np.array([q.default_dof_pos[i] for i in range(12)], np.float64)
    kw = dict(q0=q0, action_scale=q.action_scale, hip_scale_reduction=q.hip_scale_reduction, sim_dt=q.sim_dt)
    flips = total = 0
    for ct in ("T", "V"):
        if mode == 0:
            o.t["LAST_DOF_VEL"][::3] = 0.0                              # as after a reset, with the joints moving
            assert np.abs(o.t["DOF_STATE"][::3, :, 1]).max() > 0
        act = actions_for(rng, n, big=200.0 if ct == "T" else 40.0)    # action_scale is 0.25: T needs 100 N m of scaled action, V ten times its gains
        h = handle(q, o, Actuators(ct, kp, kd))
        (h.step if mode == 0 else h.physics_step)(torch.from_numpy(act).cuda()); torch.cuda.synchronize()
        clipped = ref.clip_actions(act, q.clip_actions, q.action_scale)
        # MODE 1 (the task-level tree): last_dof_vel is the velocity the step starts from (include/qa_sim_actuators.h)
        last = o.t["LAST_DOF_VEL"].copy() if mode == 0 else o.t["DOF_STATE"][..., 1].copy()
        for k in range(q.decimation):
            qk, qdk = o.t["DOF_STATE"][..., 0].copy(), o.t["DOF_STATE"][..., 1].copy()
            tau_org, big = ref.torques(ct, clipped, qk, qdk, last, kp, kd, **kw)
            tau = ref.clamp(tau_org, LIMITS)
            o.simulate(tau.astype(np.float32))
        reset = h.t["RESET"].cpu().numpy() != 0 if mode == 0 else np.zeros(n, bool)      # the fused step has re-spawned these; simulate has not
        assert reset.sum() <= n // 4 + 1, reset.sum()
        bad = np.zeros(n, bool)
        for name in ("ROOT_STATES", "DOF_STATE"):
            bad |= env_mismatch(name, h.t[name].cpu().numpy(), o.t[name], n)
        # torques of the last substep: 4 fp32 roundings of the element's largest intermediate, plus TOL of the state that substep starts from
        # through the law's coefficients (|d tau / d q| atol_q + |d tau / d qd| atol_qd; DOF_STATE has one atol for both)
        cq, cqd = ref.state_coefficients(ct, kp, kd, q.sim_dt)
        bound = 4 * ref.FP32_ROUNDING * big + (cq + cqd) * TOL["DOF_STATE"][0]
        e_org = np.abs(h.t["TORQUES_ORG"].cpu().numpy().astype(np.float64) - tau_org)
        e_tau = np.abs(h.t["TORQUES"].cpu().numpy().astype(np.float64) - tau)
        print(f"{ct} T{hf} N{n} mode{mode}: worst torque error / bound = {np.max(e_org / np.maximum(bound, 1e-300)):.3f}, max |tau_org| {np.abs(tau_org).max():.1f}, "
              f"clamped elements {int((np.abs(tau_org) > LIMITS).sum())}, resets {int(reset.sum())}")
        bad |= ((e_org > bound) | (e_tau > bound)).any(axis=1)
        assert (np.abs(tau_org) > LIMITS).any()                         # the saturating actions reach the clamp
        flips += int((bad & ~reset).sum()); total += int((~reset).sum())
        if n == 1:
            # check_flips' allowance of two env-steps would cover everything a one-env run can show: the single env is held to the bounds itself
            assert not reset.any() and not bad.any(), (ct, float(np.max(e_org / bound)), float(np.max(e_tau / bound)))
        o.arena[:] = h.arena.cpu().numpy(); o.global_step = h.global_step       # the V step starts from where the T step ended, on both sides
    return flips, total


@pytest.mark.parametrize("hf,n", [(0, 1), (0, 64), (0, 67), (1, 67)])
def test_t_and_v_laws_in_the_fused_step(hf, n):
    flips, total = run_tv(hf, n, 0)
    check_flips(f"actuators_TV_T{hf}_N{n}", flips, total, BUDGET["height_field" if hf else "plane"])


@pytest.mark.parametrize("hf,n", [(0, 67), (1, 67)])
def test_t_and_v_laws_in_the_physics_step(hf, n):
    flips, total = run_tv(hf, n, 1)
    check_flips(f"actuators_TV_phys_T{hf}_N{n}", flips, total, BUDGET["height_field" if hf else "plane"])


def test_t_law_with_zero_actions_gives_exactly_zero_torques():
    q, o, _ = pair(67, 0, 3, **OVER)
    h = handle(q, o, Actuators("T", [40.0] * 12, [1.0] * 12))
    h.t["TORQUES"].fill_(7.0); h.t["TORQUES_ORG"].fill_(7.0)
    h.step(torch.zeros(67, 12, device="cuda")); torch.cuda.synchronize()
    assert (h.t["TORQUES"] == 0).all() and (h.t["TORQUES_ORG"] == 0).all()


HELPERS_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
from tests.parity_tol import BUDGET, check_flips
from tests import test_actuators as t
what = sys.argv[2]
if what == "tv":
    flips, total = t.run_tv(0, 67, 0)
    check_flips("actuators_TV_helpers_" + sys.argv[1], flips, total, BUDGET["plane"])
elif what == "p":
    for fold in ("gains", "strength_times_gains"):
        t.run_p(0, 67, fold)
else:
    for xr in (0, 1):
        t.run_routing(0, xr)
print("CHILD_OK")
"""


@pytest.mark.parametrize("what", ["tv", "p", "routing"])
@pytest.mark.parametrize("helpers", ["0", "1"])
def test_plane_kernels_with_and_without_helper_wavefronts(helpers, what):
    """QA_ENV_HELPERS is read once per process (the pytest process takes the default: helpers on at these sizes): one child per value, each under
    its own timeout (tests/test_env_helpers.py's pattern).  Each value runs, on the plane at 67 envs, the T and V laws against the oracle's
    simulate, the P law with per-joint gains in both folds against the oracle's step, and the routing check over every lean mask with and
    without the extra rewards -- so every plane instantiation of the actuator unit, one-wavefront and with helpers, is launched and judged."""
    r = subprocess.run([sys.executable, "-c", HELPERS_CHILD % {"root": ROOT}, helpers, what], env=dict(os.environ, QA_ENV_HELPERS=helpers), timeout=300,
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD_OK" in r.stdout


# ------------------------------------------------------------------ 3. routing
def _run(h, acts):
    for a in acts:
        h.step(a)
    torch.cuda.synchronize()
    return h.arena.clone()


@pytest.mark.parametrize("hf", [0, 1])
def test_default_is_bit_identical_and_null_switches_back(hf):
    q, o, rng = pair(67, hf, 9, **OVER)
    acts = [torch.from_numpy(rng.normal(0, 0.5, (67, 12)).astype(np.float32)).cuda() for _ in range(5)]
    plain = _run(handle(q, o), acts)
    h = handle(q, o, Actuators("T", [1.0] * 12, [2.0] * 12))
    t_run = _run(h, acts)
    assert not torch.equal(t_run, plain)
    h.set_actuators(None)
    h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
    assert torch.equal(_run(h, acts), plain)
    # the uniform P model through the setter computes what cfg.kp / cfg.kd give, to rounding (the kernels contract differently): same physics
    h.set_actuators(Actuators("P", [float(q.kp)] * 12, [float(q.kd)] * 12))
    h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
    h.step(acts[0]); torch.cuda.synchronize()
    g = handle(q, o); g.step(acts[0]); torch.cuda.synchronize()
    assert not env_mismatch("DOF_STATE", h.t["DOF_STATE"].cpu().numpy(), g.t["DOF_STATE"].cpu().numpy(), 67).any()


def run_routing(hf, xr):
    from quadrupedal_agility_amd import _capi
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import ExtraRewards
    n = 67
    q, o, rng = pair(n, hf, 13, **OVER)
    act = actions_for(rng, n)
    want = ref.clamp(ref.scaled_actions(ref.clip_actions(act, q.clip_actions, q.action_scale), q.action_scale, q.hip_scale_reduction), LIMITS)
    dof = {}
    for lean in (0, 1, 3):
        for ct in (None, "T"):
            h = handle(q, o, None if ct is None else Actuators("T", [40.0] * 12, [1.0] * 12))
            if xr:
                h.set_extra_rewards(ExtraRewards([1e-30] * _capi.NUM_EXTRA_REWARDS, 0.3, 100.0, 0.02, None))
                sums = h.extra_episode_sums
            h.set_lean_exports(lean)
            h.t["TORQUES"].fill_(12345.0)
            h.step(torch.from_numpy(act).cuda()); torch.cuda.synchronize()
            dof[lean, ct] = h.t["DOF_STATE"].cpu().numpy()
            if xr:
                assert bool((sums != 0).any())
            tq = h.t["TORQUES"].cpu().numpy()
            if lean:
                assert (tq == 12345.0).all()                           # lean masks do not export the torques ...
            elif ct == "T":
                live = h.t["RESET"].cpu().numpy() == 0
                assert np.abs(tq[live].astype(np.float64) - want[live]).max() <= 2 * ref.FP32_ROUNDING * np.abs(want).max()     # the T signature
        assert (dof[lean, "T"] != dof[lean, None]).any(axis=(1, 2)).all()     # ... so the law shows in the joints: every env moved differently
        assert np.array_equal(dof[lean, "T"], dof[0, "T"])                     # and a lean mask changes nothing but the exports


@pytest.mark.parametrize("hf", [0, 1])
@pytest.mark.parametrize("xr", [0, 1])
def test_every_lean_mask_and_extra_rewards_reach_the_actuator_kernels(hf, xr):
    run_routing(hf, xr)


def test_c_side_refuses_the_self_collision_levels_and_bad_arguments():
    q, o, _ = pair(4, 0, 2, self_collision=1, **OVER)
    h = handle(q, o)
    h.set_self_collision_hips(True)
    with pytest.raises(RuntimeError, match="self_collision"):
        h.set_actuators(Actuators("T", [1.0] * 12, [1.0] * 12))
    h.set_self_collision_hips(False)
    h.set_actuators(Actuators("T", [1.0] * 12, [1.0] * 12))
    for setter in (h.set_self_collision_hips, h.set_self_collision_thighs):
        with pytest.raises(RuntimeError, match="qa_set_actuators"):
            setter(True)
    with pytest.raises(RuntimeError, match="not finite"):
        h.set_actuators(Actuators("P", [float("nan")] * 12, [1.0] * 12))


# ------------------------------------------------------------------ 4. env level, both trees
def _bbc_cfg(n):
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
    return cfg


def test_bbc_env_with_torque_control():
    from quadrupedal_agility_amd.legged_gym.envs.base import legged_robot as lr
    cfg = _bbc_cfg(16); cfg.control.control_type = "T"; cfg.domain_rand.action_delay = False
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    assert env.actuators.control_type == "T" and env.sim.actuators is env.actuators and env.p_gains.shape == (12,)
    env.reset()
    act = torch.randn(16, 12, device="cuda") * 3
    env.step(act); torch.cuda.synchronize()
    q = env.qcfg
    want = ref.clamp(ref.scaled_actions(ref.clip_actions(act.cpu().numpy(), q.clip_actions, q.action_scale), q.action_scale, q.hip_scale_reduction), LIMITS)
    live = env.reset_buf.cpu().numpy() == 0
    assert live.any() and np.abs(env.torques.cpu().numpy()[live] - want[live]).max() <= 2 * ref.FP32_ROUNDING * np.abs(want).max()


def test_tsc_env_with_per_joint_gains_constructs_and_steps():
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    cfg = Go2AgilityCfg(); cfg.env.num_envs, cfg.seed = 8, 3
    cfg.control.stiffness = {"hip": 30, "thigh": 40, "calf": 50}; cfg.control.damping = {"hip": 1.0, "thigh": 1.0, "calf": 1.0}
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    assert env.actuators.kp == [30.0, 40.0, 50.0] * 4 and env.p_gains.tolist() == [30.0, 40.0, 50.0] * 4
    env.reset()
    for _ in range(2):
        out = env.step(torch.zeros(8, 12, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(env.torques).all() and (env.torques != 0).any() and torch.isfinite(env.dof_state).all()
    assert all(torch.isfinite(x.float()).all() for x in out if torch.is_tensor(x))         # observations, rewards, resets


def test_recorded_rollout_equals_eager_and_learning_stays_finite_with_velocity_control(monkeypatch):
    """two learn() iterations at 64 envs with control_type V: the recorded rollout (hipGraph) ends in the eager one's arena, bit for bit"""
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    res = []
    for graph in ("1", "0"):
        monkeypatch.setenv("QA_ROLLOUT_GRAPH", graph)
        np.random.seed(0); torch.manual_seed(0)
        cfg = _bbc_cfg(64); cfg.control.control_type = "V"; cfg.control.stiffness = {"joint": 2.0}; cfg.control.damping = {"joint": 0.002}
        t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = False
        args = get_args(["--device", "gpu"])
        env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
        assert env.actuators.control_type == "V" and env.sim.actuators is env.actuators
        runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=None)
        losses, update = [], runner.alg.update
        runner.alg.update = lambda: (losses.append(update()), losses[-1])[1]          # what learn() hands to its logger
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        # the PPO step's six losses (surrogate, value, bounds, entropy, privileged regulariser, estimator); the discriminator's are off with AMP
        print("losses:", [list(it)[:6] for it in losses])
        assert len(losses) == 2 and all(np.isfinite(float(v)) for it in losses for v in list(it)[:6]), [list(it) for it in losses]
        assert (runner._graph is not None and not runner._graph_failed) == (graph == "1")
        assert torch.isfinite(env.sim.t["OBS"]).all() and torch.isfinite(env.sim.t["REW"]).all()
        assert all(torch.isfinite(p).all() for p in runner.alg.actor_critic.parameters())
        res.append(env.sim.arena.clone())
    assert torch.equal(res[0], res[1])
