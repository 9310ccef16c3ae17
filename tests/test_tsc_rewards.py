"""The task-level tree's fourteen extra reward terms on the GPU (include/qa_tsc_rewards.h): qa_tsc_goal_step_rewards against THE
REFERENCE'S outputs (tests/golden/tsc_rewards.npz) and against the host twin that calls the same arithmetic, the off path bit for bit
against qa_tsc_goal_step, the reset launches over 22 rows, the course env with two terms scaled, a recorded rollout against eager
steps, and the entry point's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd import _capi
from tests import tsc_env_protocol as proto
from tests.test_tsc_rewards_cpu import NB, NX, SENTINEL, TOL, assert_rew_close, descriptor, run_twin, step_inputs
from tests.test_tsc_rewards_cpu import gold, twin          # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
SIZES = (64, 67, 1)          # the fixture; the fixture tiled plus three: a ragged tail on the 64-thread block; one env


def _lib():
    return _capi.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def goal_cfg(gold, n, variant):
    slots, repeat, per, k, rows, cols = (int(v) for v in gold["const_ints"])
    delay, thr, leave, max_len, vt, border, hs = (float(v) for v in gold["scalars"])
    c = _capi.QaTscGoalCfg()
    c.num_envs, c.num_bodies, c.num_goal_slots, c.last_goal_repeat, c.goals_per_obstacle, c.num_obstacles = n, 19, slots, repeat, per, k
    c.history_len, c.history_width, c.mask_rows, c.mask_cols, c.use_camera = 5, 19, rows, cols, 0
    c.num_termination_bodies, c.num_penalised_bodies = len(gold["termination"]), len(gold["penalised"])
    for i, b in enumerate(gold["termination"]):
        c.termination_bodies[i] = int(b)
    for i, b in enumerate(gold["penalised"]):
        c.penalised_bodies[i] = int(b)
    for i, b in enumerate(gold["feet"]):
        c.feet_bodies[i] = int(b)
    c.reach_goal_delay_steps, c.next_goal_threshold, c.leave_goal_threshold, c.max_episode_length = delay, thr, leave, max_len
    c.target_lin_vel, c.border_size, c.horizontal_scale = vt, border, hs
    for i, s in enumerate(gold[f"{variant}_scale_dt"][:NB]):
        c.reward_scales[i] = float(s)
    return c


def run_kernel(gold, variant, n):
    """The fixture's four steps through qa_tsc_goal_step_rewards on env rows idx = arange(n) % 64 (envs are independent), the host-side
    reset bookkeeping between the steps as tsc_env_protocol.run_goal_steps does it.  One dict of numpy outputs per step; `idx` too."""
    lib, st = _lib(), _stream()
    idx = np.arange(n) % int(gold["num_envs"])
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                     # noqa: E731
    env_goals = gold["const_env_goals"][idx]
    const = dict(env_goals=put(env_goals), obstacle_types=put(gold["const_obstacle_types"][idx]), x_edge_mask=put(gold["const_x_edge_mask"]))
    on = gold[f"{variant}_scale_dt"][NB:] != 0
    sums = np.zeros((NB + NX, n), np.float32); sums[NB:][~on] = SENTINEL
    state = dict(episode_length=gold["const_episode_length0"][idx], cur_goal_idx=gold["const_cur_goal_idx0"][idx], reach_goal_timer=gold["const_timer0"][idx],
                 last_contacts=gold["const_last_contacts0"][idx], episode_sums=sums)
    g0 = np.clip(state["cur_goal_idx"], 0, env_goals.shape[1] - 1)
    state["cur_goals"] = env_goals[np.arange(n), g0]
    state["next_goals"] = env_goals[np.arange(n), np.clip(g0 + 1, 0, env_goals.shape[1] - 1)]
    prev = put(gold["const_last_dof_vel0"][idx])
    pact, ptorg = put(gold["const_last_actions0"][idx]), put(gold["const_last_torques_org0"][idx])
    cfg, x = goal_cfg(gold, n, variant), descriptor(gold, variant)
    results = []
    for t in range(int(gold["num_steps"])):
        dev = {k: put(v) for k, v in state.items()}
        dev.update(const)
        for k in ("root_states", "contact_forces", "rigid_body_states"):
            dev[k] = put(gold[f"in_t{t}_{k}"][idx])
        if variant != "nohist":
            dev["action_hl_history"] = put(gold[f"in_t{t}_action_hl_history"][idx])
        for k, (w, dt) in proto.OUT_SHAPES.items():
            dev[k] = put(np.zeros((n, w) if w else (n,), dt))
        io = _capi.QaTscGoalIo()
        for name in _capi.TSC_GOAL_IO_FIELDS:
            setattr(io, name, dev[name].data_ptr() if name in dev else None)
        xin = {k: put(v[idx]) for k, v in step_inputs(gold, variant, t).items()}
        for k, v in xin.items():
            setattr(x, k, v.data_ptr())
        x.prev_dof_vel, x.extra_episode_sums = prev.data_ptr(), dev["episode_sums"][NB:].data_ptr()
        x.prev_actions, x.prev_torques_org = pact.data_ptr(), ptorg.data_ptr()
        assert lib.qa_tsc_goal_step_rewards(C.byref(cfg), C.byref(io), C.byref(x), st) == 0, lib.qa_last_error()
        torch.cuda.synchronize()
        res = {k: dev[k].cpu().numpy() for k in list(proto.OUT_SHAPES) + list(proto.STATE)}
        res["prev"], res["prev_actions"], res["prev_torques_org"] = (b.cpu().numpy().copy() for b in (prev, pact, ptorg))
        state = {k: res[k].copy() for k in proto.STATE}
        ids = res["reset_buf"].astype(bool)
        state["cur_goal_idx"][ids] = 0; state["reach_goal_timer"][ids] = 0; state["episode_sums"][:, ids] = 0; state["episode_length"][ids] = 0
        state["cur_goals"][ids] = env_goals[ids, 0]; state["next_goals"][ids] = env_goals[ids, 1]
        res["sums_after_reset"] = state["episode_sums"].copy()
        results.append(res)
    return results, idx


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", ("all", "subset", "nohist"))
def test_kernel_equals_the_reference_and_the_host_twin(gold, twin, variant, n):          # noqa: F811
    results, idx = run_kernel(gold, variant, n)
    host = run_twin(twin, gold, variant)
    on = gold[f"{variant}_scale_dt"] != 0
    never_reset = np.ones(n, bool)
    for t, res in enumerate(results):
        tag = f"{variant}_t{t}_"
        sub = reference_rows(gold, tag, idx)
        # flags exactly, against the reference
        for k in ("reset_buf", "time_out_buf"):
            np.testing.assert_array_equal(res[k], sub[k], err_msg=tag + k)
        # the reward: the reference to the fixture's bound, the host twin to the tolerance the goal step holds against its oracle
        want, err = sub["rew_buf"], np.abs(res["rew_buf"] - sub["rew_buf"])
        v = gold[tag + "terms"][:, idx] * gold[f"{variant}_scale_dt"][:, None]
        assert (err <= 2e-6 * np.maximum(1.0, np.abs(v).sum(0)) + 1e-5 * np.abs(want)).all(), (tag, float(err.max()))
        np.testing.assert_allclose(res["rew_buf"], host[t]["rew"][idx], rtol=2e-6, atol=1e-6, err_msg=tag + "rew vs twin")
        # all 22 sums after the bookkeeping; rows of terms that are off are untouched
        never_reset &= sub["reset_buf"] == 0
        want_sums = np.where(on[:, None], gold[tag + "episode_sums"][:, idx], np.where(never_reset, SENTINEL, 0.0)[None, :])
        want_sums[:NB] = gold[tag + "episode_sums"][:NB, idx]
        np.testing.assert_allclose(res["sums_after_reset"], want_sums, err_msg=tag + "sums", **TOL)
        np.testing.assert_allclose(res["sums_after_reset"], host[t]["sums"][:, idx], rtol=2e-6, atol=1e-6, err_msg=tag + "sums vs twin")
        # prev_dof_vel: the reference's last_dof_vel, exactly (a copy, or zero)
        np.testing.assert_array_equal(res["prev"], gold[tag + "last_dof_vel"][idx], err_msg=tag + "prev_dof_vel")
        np.testing.assert_array_equal(res["prev"], host[t]["prev"][idx])
        # prev_actions / prev_torques_org: the reference's last_actions / last_torques_org behind the step, for every env; untouched while
        # their term is off (delta_torques in the subset: the start state stays)
        np.testing.assert_array_equal(res["prev_actions"], gold[tag + "last_actions"][idx], err_msg=tag + "prev_actions")
        np.testing.assert_array_equal(res["prev_torques_org"], (gold[tag + "last_torques_org"] if variant != "subset" else gold["const_last_torques_org0"])[idx])
    if n == 64:
        assert_rew_close(results[0]["rew_buf"], gold, variant, 0)


def reference_rows(gold, tag, idx):
    return {k: gold[tag + k][idx] for k in ("reset_buf", "time_out_buf", "rew_buf")}


class _Shim:
    """qa_tsc_goal_step_rewards under qa_tsc_goal_step's name and signature, for tests/tsc_env_protocol.run_goal_steps"""

    def __init__(self, lib, extra):
        self._lib, self._extra = lib, extra

    def qa_tsc_goal_step(self, cfg, io, stream):
        return self._lib.qa_tsc_goal_step_rewards(cfg, io, C.byref(self._extra) if self._extra is not None else None, stream)


def test_off_is_qa_tsc_goal_step_bit_for_bit():
    """extra == NULL, and a descriptor whose scales are all zero (its pointers NULL: none is looked at): every output of the eight steps
    of tests/golden/tsc_env.npz is bit-equal to qa_tsc_goal_step's"""
    fx, lib = proto.load_fixture(), _lib()
    base = proto.run_goal_steps(proto.TorchBackend(lib), fx)
    torch.cuda.synchronize()
    for extra in (None, _capi.QaTscExtraRewards()):
        got = proto.run_goal_steps(proto.TorchBackend(_Shim(lib, extra)), fx)
        assert len(got) == len(base) == 2 * proto.STEPS
        for a, b in zip(got, base):
            for k in b:
                assert a[k].tobytes() == b[k].tobytes(), k
    proto.compare_goal_steps(base, fx)


@pytest.mark.parametrize("n", SIZES)
def test_reset_launches_cover_22_rows(n):
    """qa_tsc_reset_stats / qa_tsc_reset_where with num_terms = 22 against the torch expression of LeggedRobot._reset's CPU branch"""
    g = torch.Generator().manual_seed(n)
    rows, slots = NB + NX, 26
    sums = torch.randn(rows, n, generator=g).cuda()
    flags = (torch.rand(n, generator=g) < 0.4).to(torch.uint8).cuda()
    if n != 64:
        flags[-min(n, 3):] = 1                                           # the ragged tail (the one env) resets
    max_len_s = 20.0
    for f in (flags, torch.zeros_like(flags)):                            # some reset; nobody resets (the means are kept)
        means = torch.full((rows,), 3.0, device="cuda")
        any_reset = torch.zeros(1, dtype=torch.uint8, device="cuda")
        _capi.API.launch("tsc_reset_stats", f.data_ptr(), sums.data_ptr(), n, rows, max_len_s, means.data_ptr(), any_reset.data_ptr(), on=f)
        ff = (f != 0).to(torch.float32)
        cnt = ff.sum()
        want = torch.where(cnt > 0, (sums * ff).sum(dim=1) / torch.clamp(cnt, min=1.0) / max_len_s, torch.full_like(means, 3.0))
        assert torch.allclose(means, want, rtol=1e-5, atol=1e-6) and int(any_reset) == int(cnt > 0)
        env_goals = torch.randn(n, slots, 3, generator=g).cuda()
        idx, timer = torch.randint(0, slots, (n,), generator=g).cuda(), torch.rand(n, generator=g).cuda()
        ep, start = torch.randint(1, 50, (n,), generator=g).cuda(), torch.zeros(n, dtype=torch.long, device="cuda")
        cur, nxt = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
        obst_idx = torch.zeros(n, dtype=torch.long, device="cuda")
        s2, idx0, timer0, ep0 = sums.clone(), idx.clone(), timer.clone(), ep.clone()
        _capi.API.launch("tsc_reset_where", f.data_ptr(), any_reset.data_ptr(), start.data_ptr(), idx.data_ptr(), timer.data_ptr(), s2.data_ptr(), rows,
                         ep.data_ptr(), env_goals.data_ptr(), slots, cur.data_ptr(), nxt.data_ptr(), None, 0.0, obst_idx.data_ptr(), None, n, on=f)
        m = f != 0
        assert torch.equal(s2, sums * (~m).to(sums.dtype).unsqueeze(0))                  # TaskLevelBookkeeping.reset_where, every row
        assert torch.equal(idx, torch.where(m, start, idx0)) and torch.equal(timer, timer0 * (~m)) and torch.equal(ep, ep0 * (~m))
        gi = idx.clamp(0, slots - 1)
        assert torch.equal(cur, env_goals[torch.arange(n), gi]) and torch.equal(nxt, env_goals[torch.arange(n), (gi + 1).clamp(0, slots - 1)])


def _course_env(n, seed, **scales):
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from tests.test_tsc_course_env import make_cfg
    cfg = make_cfg(n, seed, env__episode_length_s=0.3)                    # 15-step episodes: resets among the steps
    for k, v in scales.items():
        setattr(cfg.rewards.scales, k, v)
    return lr.LeggedRobot(cfg, sim_device="cuda:0")


def test_course_env_with_torques_and_dof_acc_scaled():
    """64 envs (the smallest env count tests/test_tsc_course_env.py builds on the GPU): the scaled terms reach rew_buf, extras and the sums.
    A third env with action_rate and delta_torques scaled shows what stands in for the reference's last_actions / last_torques_org: in front
    of step t + 1 the goal step's own buffers hold step t's `actions` / `torques_org` for EVERY env, as :279 and :281 leave them, while the
    arena's LAST_ACTIONS / LAST_TORQUES_ORG have lost the rows of the envs that reset at t (that check is what sent the two to owned buffers)."""
    n, steps = 64, 24
    torch.manual_seed(0)
    env = _course_env(n, 3, torques=-2e-3, dof_acc=-2.5e-6)
    torch.manual_seed(0)
    ref = _course_env(n, 3)
    torch.manual_seed(0)
    env2 = _course_env(n, 3, action_rate=-0.5, delta_torques=-1e-3)
    assert list(env.episode_sums) == sorted(list(_capi.TSC_REWARD_NAMES[:-1]) + ["torques", "dof_acc"]) + ["termination"] and len(env.episode_sums) == 10
    assert set(env.reward_scales) == set(env.episode_sums) and len(ref.episode_sums) == 8 and ref.bk.episode_sums_buf.shape[0] == 8
    assert env.bk.episode_sums_buf.shape == (22, n) and env._episode_means.shape == (22,)
    assert env.dof_pos_limits.shape == (12, 2) and env.dof_vel_limits.shape == (12,) and env.torque_limits.shape == (12,) and env.hip_indices.tolist() == [0, 3, 6, 9]
    g = torch.Generator().manual_seed(5)
    resets, differs, snap, arena_lost_rows = 0, False, None, False
    for k in range(steps):
        a = (torch.randn(n, 12, generator=g) * 0.8).cuda()
        hist = torch.randn(n, 8, 19, generator=g).cuda()
        sums_before = {name: env2.episode_sums[name].clone() for name in ("action_rate", "delta_torques")}
        for e in (env, ref, env2):
            e.step(a, hist)
        torch.cuda.synchronize()
        reset = env2.reset_buf != 0
        if snap is not None:
            # what step k read as "last" is step k - 1's snapshot, resets among them or not: the terms it added say so
            keep = ~reset
            want = dict(action_rate=env2.reward_scales["action_rate"] * torch.norm(snap[0] - env2.actions, dim=1),
                        delta_torques=env2.reward_scales["delta_torques"] * torch.sum(torch.square(env2.torques_org - snap[1]), dim=1))
            for name, w in want.items():
                got = env2.episode_sums[name] - sums_before[name]
                tol = 2e-6 * torch.clamp(sums_before[name].abs() + w.abs(), min=1.0) + 1e-5 * w.abs()
                assert ((got - w).abs()[keep] <= tol[keep]).all(), (k, name)
            arena_lost_rows |= bool(prev_reset.any() and not torch.equal(last_arena[0], snap[0]))
        # ... and the buffers now hold this step's tensors for every env
        assert torch.equal(env2.bk.prev_actions, env2.actions) and torch.equal(env2.bk.prev_torques_org, env2.torques_org), k
        snap, prev_reset = (env2.actions.clone(), env2.torques_org.clone()), reset.clone()
        last_arena = (env2.last_actions.clone(), env2.last_torques_org.clone())
        resets += int((env.reset_buf != 0).sum())
        # the same physics on the same seed (the terms change rewards only), and a reward that differs where the penalties bite
        assert torch.equal(env.root_states, ref.root_states) and torch.equal(env.reset_buf, ref.reset_buf) and torch.equal(env2.root_states, ref.root_states)
        differs |= not torch.equal(env.rew_buf, ref.rew_buf)
        assert (env.rew_buf <= ref.rew_buf + 1e-6).all()                  # two penalties: never more reward
        # prev_dof_vel is dof_vel as the goal step saw it, zero for the envs it reset
        assert (env.bk.prev_dof_vel[env.reset_buf != 0] == 0).all()
    assert resets >= n and differs and arena_lost_rows
    assert set(env.extras["episode"]) == {"rew_" + k for k in _capi.TSC_REWARD_NAMES} | {"rew_torques", "rew_dof_acc"}
    assert set(ref.extras["episode"]) == {"rew_" + k for k in _capi.TSC_REWARD_NAMES}
    assert float(env.extras["episode"]["rew_torques"]) < 0 and float(env.extras["episode"]["rew_dof_acc"]) < 0
    assert all("rew_" + k in env.extras["episode"] for k in env.reward_scales)


def test_recorded_rollout_equals_eager_steps_with_the_terms_on(tmp_path):
    """the teacher's rollout as one hipGraph replay per iteration (QA_TSC_ROLLOUT_GRAPH's default) against the eager loop of the same job, 64
    envs, three iterations (eager warm-up, recording, one replay): the stored rollout and the extra terms' state are identical"""
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import class_to_dict
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfgPPO
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    from tests.test_tsc_course_env import make_cfg
    out = {}
    for mode in ("recorded", "eager"):
        torch.manual_seed(0)
        cfg = make_cfg(64, 1, env__episode_length_s=0.5, domain_rand__push_robots=True, obstacle__randomize_start=True, domain_rand__push_interval=7)
        cfg.rewards.scales.torques, cfg.rewards.scales.dof_acc, cfg.rewards.scales.action_rate = -2e-3, -2.5e-6, -0.1
        env = lr.LeggedRobot(cfg, sim_device="cuda:0")
        runner = OnPolicyRunner(env, class_to_dict(Go2AgilityCfgPPO()), log_dir=str(tmp_path / mode), device="cuda:0")
        assert runner.use_rollout_graph                                   # the default
        runner.use_rollout_graph = mode == "recorded"
        snaps = []
        for it in range(3):
            runner.learn(1, init_at_random_ep_len=(it == 0))
            st = runner.alg.storage
            snaps.append(dict(rewards=st.rewards.clone(), dones=st.dones.clone(), obs=st.observations.clone(), sums=env.bk.episode_sums_buf.clone(),
                              prev=env.bk.prev_dof_vel.clone(), means=env._episode_means.clone(), root=env.root_states.clone()))
        if mode == "recorded":
            assert any(isinstance(v, tuple) for v in runner._rollout_graphs.values())
        out[mode] = snaps
    for it in range(3):
        for k in out["eager"][it]:
            assert torch.equal(out["eager"][it][k], out["recorded"][it][k]), (it, k)
    r = out["recorded"][-1]
    assert (r["sums"][8:] != 0).any() and (r["means"][8:] != 0).sum() == 3 and r["dones"].float().mean().item() > 0.005


def test_entry_point_refuses_a_missing_pointer_and_misaligned_rows(gold):          # noqa: F811
    lib, st = _lib(), _stream()
    n = 64
    fx = proto.load_fixture()
    be = proto.TorchBackend(lib)
    cfg = proto.goal_cfg(fx, n, 0)
    tag = "goal_c0_t0_"
    dev = {k: be.put(v) for k, v in dict(
        root_states=fx[tag + "root_states"], contact_forces=fx[tag + "contact_forces"], rigid_body_states=fx[tag + "rigid_body_states"],
        env_goals=fx["goal_env_goals"], obstacle_types=fx["goal_obstacle_types"].astype(np.int64), x_edge_mask=fx["goal_x_edge_mask"].astype(np.uint8),
        episode_length=fx["goal_episode_length0"].astype(np.int64), cur_goal_idx=fx["goal_cur_goal_idx0"].astype(np.int64),
        reach_goal_timer=fx["goal_timer0"].astype(np.float32), last_contacts=fx["goal_last_contacts0"].astype(np.uint8),
        cur_goals=fx["goal_cur_goals0"].astype(np.float32), next_goals=fx["goal_next_goals0"].astype(np.float32)).items()}
    dev["episode_sums"] = torch.zeros(NB + NX, n, device="cuda")
    for k, (w, dt) in proto.OUT_SHAPES.items():
        dev[k] = be.put(np.zeros((n, w) if w else (n,), dt))
    io = _capi.QaTscGoalIo()
    for name in _capi.TSC_GOAL_IO_FIELDS:
        setattr(io, name, dev[name].data_ptr() if name in dev else None)
    bufs = {k: torch.zeros(n * 24 + 8, device="cuda") for k in _capi.TSC_EXTRA_POINTERS[:6]}

    def call(on, missing=None, shifted=None, no_sums=False):
        x = descriptor(gold, "all", scale_dt=[(-0.1 if name in on else 0.0) for name in _capi.TSC_EXTRA_REWARD_NAMES])
        for k, t in bufs.items():
            setattr(x, k, None if k == missing else t.data_ptr() + (4 if k == shifted else 0))
        x.extra_episode_sums = None if no_sums else dev["episode_sums"][NB:].data_ptr()
        rc = lib.qa_tsc_goal_step_rewards(C.byref(cfg), C.byref(io), C.byref(x), st)
        return rc, lib.qa_last_error().decode()

    needs = {"action_rate": ("actions", "prev_actions"), "delta_torques": ("torques_org", "prev_torques_org"), "torques": ("torques_org",),
             "torque_limits": ("torques_org",), "dof_acc": ("dof_state", "prev_dof_vel"), "dof_error": ("dof_state",), "dof_pos_limits": ("dof_state",),
             "dof_vel_limits": ("dof_state",), "hip_pos": ("dof_state",)}
    for term, ptrs in needs.items():
        for p in ptrs:
            rc, msg = call({term}, missing=p)
            assert rc == -1 and p in msg and "null" in msg, (term, p, msg)
            rc, msg = call({term}, shifted=p)
            assert rc == -1 and p in msg and "aligned" in msg, (term, p, msg)
    rc, msg = call({"every_step"}, no_sums=True)
    assert rc == -1 and "extra_episode_sums" in msg
    # a term that is off needs nothing: every_step alone runs with every row pointer NULL, and a misaligned pointer nobody reads is no error
    assert call({"every_step"}, missing="dof_state")[0] == 0 and call({"lin_vel_z", "feet_stumble"}, shifted="actions")[0] == 0
    torch.cuda.synchronize()
    assert call(set(_capi.TSC_EXTRA_REWARD_NAMES))[0] == 0
    torch.cuda.synchronize()
