#!/usr/bin/env python3
"""tests/golden/tsc_rewards.npz: the task-level tree's 22 reward terms as THE REFERENCE'S OWN PYTHON computes them.

Build container only (needs the reference checkout, like tools/gen_golden_tsc_env.py whose stub env this reuses).  64 envs, 4 consecutive
calls of the reference's LeggedRobot.post_physics_step on synthetic simulator tensors, with all fourteen extra scales set and the eight at
their config values, every _reward_* function wrapped to record what it returned.  The stub's reset_idx additionally does what the
simulator side of the reference's reset_idx does to the inputs of these terms: dof_vel[ids] = 0 (_reset_dofs) and :387-389.  The inputs are
edited so that every branch of every term occurs (asserted below).  Three variants on the same inputs: "all", "subset" (torques, dof_acc,
action_rate only) and "nohist" (all, without the task policy's action history).  Only inputs and the reference's outputs are written.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden_tsc_env as ge                                                   # noqa: E402  (imports the reference)
from quadrupedal_agility_amd import _capi, go2_limits                             # noqa: E402

N, STEPS = 64, 4
T = ge.T
BASE, EXTRA = list(_capi.TSC_REWARD_NAMES), list(_capi.TSC_EXTRA_REWARD_NAMES)
# each scaled term (scale * dt * term) is O(1) or less on these inputs
SCALES = dict(action_rate=-0.5, ang_vel_xy=-1.0, delta_torques=-1e-3, dof_acc=-2.5e-7, dof_error=-0.5, dof_pos_limits=-10.0, dof_vel_limits=-5.0,
              every_step=15.0, feet_stumble=-2.0, hip_pos=-1.0, lin_vel_z=-2.0, orientation=-1.0, torque_limits=-0.2, torques=-1e-3)
VARIANTS = (("all", SCALES, True), ("subset", {k: SCALES[k] for k in ("torques", "dof_acc", "action_rate")}, True), ("nohist", SCALES, False))
FEET = [6, 10, 14, 18]
DEFAULT = np.array([0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5], np.float32)


def make_inputs(cfg):
    """the constants, the start state and the four steps' simulator tensors -- shared by the variants"""
    rng = np.random.default_rng(20251019)
    ge.rng = rng                                                                  # random_quats draws from the module's generator
    K, G = 6, cfg.obstacle.num_goals
    slots = K * G + cfg.obstacle.last_goal_repeat
    env_goals = np.zeros((N, slots, 3), np.float32)
    env_goals[:, :, 0] = np.arange(slots)[None, :] * 1.5 + rng.uniform(-0.2, 0.2, (N, slots))
    env_goals[:, :, 1] = rng.uniform(-1.0, 1.0, (N, slots))
    env_goals[:, K * G:, :] = env_goals[:, K * G - 1: K * G, :]
    idx0 = rng.integers(0, slots - 1, N); idx0[:8] = slots - cfg.obstacle.last_goal_repeat - 1
    timer0 = rng.integers(0, 3, N).astype(np.float32); timer0[:8] = 2.0
    ep0 = rng.integers(0, 1990, N); ep0[-6:] = int(np.ceil(cfg.env.episode_length_s / (cfg.control.decimation * cfg.sim.dt))) - 1
    rows, cols = 260, 140
    const = dict(env_goals=env_goals, obstacle_types=rng.integers(0, 6, (N, K)).astype(np.int64), cur_goal_idx0=idx0.astype(np.int64), timer0=timer0,
                 episode_length0=ep0.astype(np.int64), last_contacts0=(rng.random((N, 4)) < 0.3).astype(np.uint8),
                 x_edge_mask=(rng.random((rows, cols)) < 0.25).astype(np.uint8),
                 last_actions0=rng.normal(0, 1, (N, 12)).astype(np.float32), last_dof_vel0=rng.normal(0, 6, (N, 12)).astype(np.float32),
                 last_torques_org0=rng.normal(0, 6, (N, 12)).astype(np.float32), default_dof_pos=DEFAULT,
                 ints=np.array([slots, cfg.obstacle.last_goal_repeat, G, K, rows, cols], np.int32))
    lim = go2_limits.soft_dof_pos_limits(cfg.rewards.soft_dof_pos_limit).numpy()
    vlim = (torch.tensor(go2_limits.DOF_VEL_LIMITS) * cfg.rewards.soft_dof_vel_limit).numpy()
    tlim = (torch.tensor(go2_limits.TORQUE_LIMITS) * cfg.rewards.soft_torque_limit).numpy()
    steps = []
    for t in range(STEPS):
        s = dict(u_xy=rng.normal(0, 1, (N, 2)), spread=rng.choice([0.2, 1.5, 6.0], N, p=[0.4, 0.45, 0.15])[:, None], z=rng.uniform(0.2, 0.5, N),
                 quat=ge.random_quats(N), vel=rng.normal(0, 1.0, (N, 6)), rb_xy=rng.uniform(-0.4, 0.4, (N, 19, 2)))
        cf = rng.normal(0, 3.0, (N, 19, 3)).astype(np.float32) * (rng.random((N, 19, 1)) < 0.03)
        cf[:, FEET] = np.abs(rng.normal(0, 8.0, (N, 4, 3))) * np.array([0.1, 0.1, 1.0]) * (rng.random((N, 4, 1)) < 0.6)     # mostly vertical: no stumble
        o = 12 * t                                                               # the edited envs move from step to step
        cf[o + 10, FEET[1]] = [30.0, 5.0, 3.0]; cf[o + 11, FEET[2]] = [0.0, -9.0, 2.0]                                       # stumbling feet
        hist = rng.normal(0, 0.7, (N, 5, 19)).astype(np.float32); hist[:, :, 0] = rng.integers(0, 3, (N, 5))
        q = (DEFAULT[None] + rng.normal(0, 0.3, (N, 12))).astype(np.float32)
        q = np.clip(q, lim[None, :, 0] + 0.02, lim[None, :, 1] - 0.02)
        q[o + 0] = lim[:, 0] - 0.1; q[o + 1] = lim[:, 0] - np.linspace(0.01, 0.3, 12)                                      # every joint past its lower limit
        q[o + 2] = lim[:, 1] + 0.1; q[o + 3] = lim[:, 1] + np.linspace(0.01, 0.3, 12)                                      # ... and past its upper one
        qd = np.clip(rng.normal(0, 6, (N, 12)), -15, 15).astype(np.float32)                                                 # below the limit: clip -> 0
        qd[o + 4] = (vlim + 0.5) * np.where(np.arange(12) % 2, 1, -1); qd[o + 5, :6] = vlim[:6] + 0.25                      # inside (0, 1)
        qd[o + 6] = -(vlim + 5.0); qd[o + 7, 6:] = vlim[6:] + 3.0                                                           # past 1
        tq = rng.normal(0, 6, (N, 12)).astype(np.float32)
        tq[o + 8] = tlim + 4.0; tq[o + 9] = -(tlim + 9.0)
        s.update(contact_forces=cf.astype(np.float32), action_hl_history=hist, dof_pos=q.astype(np.float32), dof_vel=qd.astype(np.float32),
                 actions=rng.normal(0, 1, (N, 12)).astype(np.float32), torques_org=tq.astype(np.float32))
        steps.append(s)
    return const, steps, dict(lower=lim[:, 0], upper=lim[:, 1], vel=vlim, torque=tlim)


def run_variant(scales, with_hist, const, steps, limits):
    env, cfg = ge.make_env()
    for k in EXTRA:
        env.reward_scales[k] = scales.get(k, 0.0)
    env._prepare_reward_function()
    env.env_goals, env.obstacle_types = T(const["env_goals"]), T(const["obstacle_types"], torch.long)
    env.cur_goal_idx, env.reach_goal_timer = T(const["cur_goal_idx0"], torch.long), T(const["timer0"])
    env.cur_goals, env.next_goals = env._gather_cur_goals(), env._gather_cur_goals(future=1)
    env.episode_length_buf, env.last_contacts = T(const["episode_length0"], torch.long), T(const["last_contacts0"], torch.bool)
    env.x_edge_mask = T(const["x_edge_mask"], torch.bool)
    env.commands = torch.zeros(N, 5)
    for name in ("base_quat", "base_lin_vel", "base_ang_vel", "projected_gravity"):
        setattr(env, name, torch.zeros(N, 4 if name == "base_quat" else 3))
    env.last_root_vel, env.rew_buf = torch.zeros(N, 6), torch.zeros(N)
    env.last_actions, env.last_dof_vel, env.last_torques_org = T(const["last_actions0"]), T(const["last_dof_vel0"]), T(const["last_torques_org0"])
    env.default_dof_pos = T(DEFAULT[None])
    env.dof_pos_limits = go2_limits.soft_dof_pos_limits(cfg.rewards.soft_dof_pos_limit)
    env.dof_vel_limits, env.torque_limits = torch.tensor(go2_limits.DOF_VEL_LIMITS), torch.tensor(go2_limits.TORQUE_LIMITS)
    env.hip_indices = torch.tensor(go2_limits.HIP_INDICES)
    base_reset = env.reset_idx

    def reset_idx(ids):                      # + the simulator side of reset_idx for these terms' inputs: _reset_dofs zeroes dof_vel, :387-389
        env.dof_vel[ids] = 0.
        env.last_actions[ids] = 0.
        env.last_dof_vel[ids] = 0.
        env.last_torques_org[ids] = 0.
        base_reset(ids)
    env.reset_idx = reset_idx
    raw = {}

    def record(name, fn):
        def call():
            r = fn()
            raw[name] = (r.clone().float() if torch.is_tensor(r) else torch.full((N,), float(r)))
            return r
        return call
    env.reward_functions = [record(n, getattr(env, "_reward_" + n)) for n in env.reward_names]
    env._reward_termination = record("termination", env._reward_termination)
    out = {"reward_names": np.array(env.reward_names), "scale_dt": np.array([env.reward_scales.get(n, 0.0) for n in BASE + EXTRA], np.float64)}
    for t, s in enumerate(steps):
        root = np.zeros((N, 13), np.float32)
        root[:, :2] = env.cur_goals.numpy()[:, :2] + s["u_xy"] * s["spread"]
        root[:, 2] = s["z"]; root[N // 2: N // 2 + 5, 2] = -0.3
        root[:, 3:7], root[:, 7:13] = s["quat"], s["vel"]
        rb = np.zeros((N, 19, 13), np.float32); rb[:, :, :2] = root[:, None, :2] + s["rb_xy"]
        env.root_states, env.contact_forces, env.rigid_body_states = T(root), T(s["contact_forces"]), T(rb)
        env.action_hl_history_buf = T(s["action_hl_history"]) if with_hist else None
        env.dof_pos, env.dof_vel, env.actions, env.torques_org = T(s["dof_pos"]), T(s["dof_vel"]), T(s["actions"]), T(s["torques_org"])
        before = dict(last_actions=env.last_actions.numpy().copy(), last_torques_org=env.last_torques_org.numpy().copy(),
                      last_dof_vel=env.last_dof_vel.numpy().copy())
        raw.clear()
        env.post_physics_step()
        zero = np.zeros(N, np.float32)
        out.update({f"t{t}_{k}": v for k, v in dict(
            root_states=root, rigid_body_states=rb, in_last_actions=before["last_actions"], in_last_torques_org=before["last_torques_org"],
            in_last_dof_vel=before["last_dof_vel"], terms=np.stack([raw[n].numpy() if n in raw else zero for n in BASE + EXTRA]),
            base_lin_vel=env.base_lin_vel.numpy().copy(), base_ang_vel=env.base_ang_vel.numpy().copy(), projected_gravity=env.projected_gravity.numpy().copy(),
            rew_buf=env.rew_buf.numpy().copy(), reset_buf=env.reset_buf.numpy().astype(np.uint8), time_out_buf=env.time_out_buf.numpy().astype(np.uint8),
            episode_sums=np.stack([env.episode_sums[n].numpy().copy() if n in env.episode_sums else zero for n in BASE + EXTRA]),
            last_dof_vel=env.last_dof_vel.numpy().copy(), last_actions=env.last_actions.numpy().copy(),
            last_torques_org=env.last_torques_org.numpy().copy()).items()})
    return out, dict(dt=env.dt, max_episode_length=env.max_episode_length, cfg=cfg)


def coverage(flat, limits, variant="all"):
    """every branch occurs, each in at least two envs; repeated on the stored data by tests/test_tsc_rewards_cpu.py"""
    names = BASE + EXTRA
    sd = flat[f"{variant}_scale_dt"]
    seen_zeroing = False
    for t in range(STEPS):
        q, qd, tq, cf = (flat[f"in_t{t}_{k}"] for k in ("dof_pos", "dof_vel", "torques_org", "contact_forces"))
        assert ((q < limits["lower"]).sum(0) >= 2).all() and ((q > limits["upper"]).sum(0) >= 2).all(), "a joint past each soft position limit"
        over = np.abs(qd) - limits["vel"]
        assert (over < 0).any(1).sum() >= 2 and ((over > 0) & (over < 1)).any(1).sum() >= 2 and (over > 1).any(1).sum() >= 2, "three regions of clip(0, 1)"
        assert (np.abs(tq) > limits["torque"]).any(1).sum() >= 2 and (np.abs(tq) < limits["torque"]).any(1).sum() >= 2
        terms = dict(zip(names, flat[f"{variant}_t{t}_terms"]))
        assert (terms["feet_stumble"] == 1).sum() >= 2 and (terms["feet_stumble"] == 0).sum() >= 2
        assert (terms["dof_pos_limits"] > 0).sum() >= 4 and (terms["dof_vel_limits"] > 0).sum() >= 4 and (terms["torque_limits"] > 0).sum() >= 2
        pre = (flat[f"{variant}_t{t}_terms"][np.array(names) != "termination"] * sd[np.array(names) != "termination", None]).sum(0)
        assert (pre < 0).sum() >= 2 and (pre > 0).sum() >= 2, "a negative total before the clip"
        assert ((pre < 0) & (terms["termination"] > 0)).sum() >= 2, "termination on top of a negative total"
        assert flat[f"{variant}_t{t}_reset_buf"].sum() >= 4 and (flat[f"{variant}_t{t}_reset_buf"] == 0).sum() >= 4
        if t > 0:
            was_reset = flat[f"{variant}_t{t - 1}_reset_buf"].astype(bool)
            assert (flat[f"{variant}_t{t}_in_last_dof_vel"][was_reset] == 0).all()
            assert (flat[f"{variant}_t{t}_in_last_dof_vel"][~was_reset] == flat[f"in_t{t - 1}_dof_vel"][~was_reset]).all()
            # dof_acc of the envs that reset one step earlier: previous velocity zeroed (the reference) against not zeroed
            inv = 1.0 / flat["dt"]
            not_zeroed = (((flat[f"in_t{t - 1}_dof_vel"] - qd) * inv) ** 2).sum(1)
            seen_zeroing |= bool((np.abs(not_zeroed - terms["dof_acc"])[was_reset] > 1e-3 * terms["dof_acc"][was_reset]).all() and was_reset.sum() >= 2)
    assert sum(int(flat[f"{variant}_t{t}_time_out_buf"].sum()) for t in range(STEPS)) >= 2, "time-outs: a reset without the termination term"
    assert seen_zeroing, "a reset followed by a step whose dof_acc depends on the zeroing"


def main():
    _, cfg0 = ge.make_env()
    const, steps, limits = make_inputs(cfg0)
    flat = {"num_envs": np.array(N), "num_steps": np.array(STEPS), "feet": np.array(FEET, np.int32)}
    flat.update({"const_" + k: v for k, v in const.items()})
    flat.update({"limit_" + k: v.astype(np.float32) for k, v in limits.items()})
    for t, s in enumerate(steps):
        flat.update({f"in_t{t}_{k}": s[k] for k in ("contact_forces", "action_hl_history", "dof_pos", "dof_vel", "actions", "torques_org")})
    for variant, scales, with_hist in VARIANTS:
        out, info = run_variant(scales, with_hist, const, steps, limits)
        flat.update({f"{variant}_{k}": v for k, v in out.items()})
        if variant == "all":
            for t in range(STEPS):                                               # the simulator tensors that follow the goals: the same in every variant
                flat[f"in_t{t}_root_states"], flat[f"in_t{t}_rigid_body_states"] = out[f"t{t}_root_states"], out[f"t{t}_rigid_body_states"]
        else:
            for t in range(STEPS):
                assert np.array_equal(out[f"t{t}_root_states"], flat[f"in_t{t}_root_states"]) and np.array_equal(out[f"t{t}_reset_buf"], flat[f"all_t{t}_reset_buf"])
        for t in range(STEPS):
            del flat[f"{variant}_t{t}_root_states"], flat[f"{variant}_t{t}_rigid_body_states"]
    cfg = info["cfg"]
    flat.update(dt=np.array(info["dt"]), base_names=np.array(BASE), extra_names=np.array(EXTRA),
                term_names=np.array(BASE + EXTRA), termination=np.array(ge.make_env()[0].termination_contact_indices.numpy(), np.int32),
                penalised=np.array(ge.make_env()[0].penalised_contact_indices.numpy(), np.int32),
                scalars=np.array([cfg.env.reach_goal_delay / info["dt"], cfg.env.next_goal_threshold, cfg.env.leave_goal_threshold, info["max_episode_length"],
                                  cfg.rewards.target_lin_vel, cfg.obstacle.border_size, cfg.obstacle.horizontal_scale], np.float64),
                soft_limits=np.array([cfg.rewards.soft_dof_pos_limit, cfg.rewards.soft_dof_vel_limit, cfg.rewards.soft_torque_limit], np.float64))
    coverage(flat, limits)
    path = os.path.join(ROOT, "tests", "golden", "tsc_rewards.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes,", len(flat), "arrays; walk", list(flat["all_reward_names"]))
    print("resets", [int(flat[f"all_t{t}_reset_buf"].sum()) for t in range(STEPS)], "subset names", list(flat["subset_reward_names"]))


if __name__ == "__main__":
    main()
