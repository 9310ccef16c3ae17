"""Obstacle curriculum of the agility course (include/qa_tsc_curriculum.h): the reference's `_update_obstacle_curriculum`
(tsc/legged_gym/envs/base/legged_robot.py:917-957) as one launch of the env step, decided on the device.

CPU: the torch restatement (`ObstacleCurriculum.update_torch`) against the reference's own outputs (tests/golden/obstacle_curriculum.npz,
written by tools/gen_golden_obstacle_curriculum.py), the trigger's truth table, the float64 increment tables, arming, the data-parallel
success rate.  GPU: the kernel against the restatement bit for bit, the HIP env against the oracle-backend env across a raise, a recorded
rollout against an eager one across a raise, a logged run."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from quadrupedal_agility_amd import _capi
from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import class_to_dict
from quadrupedal_agility_amd.tsc.legged_gym import obstacle_curriculum as oc
from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg, Go2AgilityCfgPPO
from quadrupedal_agility_amd.tsc.legged_gym.utils.obstacle import NO_CEILING, Obstacle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obstacle_curriculum.npz")
_COURSES = {}


def course(n, seed=11):
    """one curriculum course per (n, seed) for the whole module (building it is the slow part; nobody writes to it)"""
    if (n, seed) not in _COURSES:
        cfg = Go2AgilityCfg()
        cfg.obstacle.curriculum = True
        _COURSES[(n, seed)] = Obstacle(cfg.obstacle, n, seed=seed)
    return _COURSES[(n, seed)]


def make(ob, period, device, two_maps=True):
    """an ObstacleCurriculum over fresh copies of the course's tensors -> (curriculum, dict of the tensors)"""
    cur = oc.ObstacleCurriculum.from_course(ob, period, device)
    T = lambda a, dt: torch.from_numpy(np.array(a)).to(device, dt).contiguous()       # noqa: E731  (np.array: a copy, the course is shared)
    t = dict(height=T(ob.height_field_raw, torch.int16), scan=T(ob.height_field_raw, torch.int16) if two_maps else None,
             ceiling=T(ob.ceiling_raw, torch.int16), goals=T(ob.flat_goals(), torch.float32))
    cur.bind(t["height"], t["scan"], t["ceiling"], t["goals"])
    return cur, t


def twin_step(cur, gc, rate, any_reset=1):
    cur.set_rate(rate)
    dev = cur.state.device
    cur.update_torch(torch.tensor([gc], dtype=torch.int64, device=dev), torch.tensor([any_reset], dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ CPU
def test_generator_outputs_are_unchanged_and_the_tyre_ceiling_is_recorded():
    """the new field marks the tyre's cells of the ceiling only; the tunnel roof shares the field and is not in it"""
    ob = course(4)
    roofed = ob.ceiling_raw != NO_CEILING
    assert ob.tire_ceiling_mask.dtype == bool and ob.tire_ceiling_mask.shape == ob.ceiling_raw.shape
    assert (ob.tire_ceiling_mask & ~roofed).sum() == 0
    tyre, tunnel = int(ob.tire_ceiling_mask.sum()), int((roofed & ~ob.tire_ceiling_mask).sum())
    assert tyre > 4 * 20 and tunnel > 4 * 200, (tyre, tunnel)
    # the tyre's ceiling lies over the tyre's movable floor cells (same rectangle of the same stamp)
    assert (ob.tire_ceiling_mask & ob.tire_jump_mask).sum() > 0.8 * tyre


def test_twin_reproduces_the_reference():
    g = np.load(GOLD)
    ob = course(int(g["num_envs"]), int(g["seed"]))
    cell_index = g["cell_index"]
    assert np.array_equal(ob.height_field_raw.reshape(-1)[cell_index], g["built_cells"])
    assert np.array_equal(ob.flat_goals().astype(np.float32).view(np.uint32), g["built_goals"].view(np.uint32))
    cur, t = make(ob, int(2 * float(g["max_episode_length"])), "cpu")
    assert cur.threshold == float(g["curr_threshold"]) and cur.last == int(g["count_at_cap"]) + 1
    built_ceiling = t["ceiling"].clone()
    tyre_inc = {0: 0}
    rep_y = np.zeros(g["built_goals"].shape, bool)
    rep_y[:, -ob.last_goal_repeat:, 1] = True
    for i, (rate, counter, init_done, count_before) in enumerate(g["calls"]):
        assert init_done == 1
        cur.state[0] = int(count_before)
        twin_step(cur, int(counter), float(rate))
        count, bar, tyre, _ = cur.read_state()
        want = g[f"call_{i}_state"]
        for m in (t["height"], t["scan"]):
            flat = m.numpy().reshape(-1)
            assert np.array_equal(flat[cell_index], g[f"call_{i}_cells"]), i
            assert int(flat.astype(np.int64).sum() - flat[cell_index].astype(np.int64).sum()) == int(g[f"call_{i}_rest_sum"])
        got, ref = t["goals"].numpy(), g[f"call_{i}_goals"]
        assert np.array_equal(got[~rep_y].view(np.uint32), ref[~rep_y].view(np.uint32)), i
        # the y of the last goal's repeats is not the curriculum's: a raise leaves this build's value (float64 sum, then fp32) where the
        # reference re-derives its own (fp32 sum) -- one ulp apart from the constructor on, with or without a raise
        assert np.array_equal(got[rep_y].view(np.uint32), g["built_goals"][rep_y].view(np.uint32))
        assert np.abs(got[rep_y].view(np.int32) - ref[rep_y].view(np.int32)).max() <= 1
        assert count == int(want[0])
        if count:
            assert bar == want[1] and tyre == want[2]            # exact: the same float64 expression
            tyre_inc[count] = int(tyre / float(g["vertical_scale"]))
            moved = t["ceiling"] - built_ceiling
            mask = torch.from_numpy(ob.tire_ceiling_mask)
            assert (moved[mask] == tyre_inc[count]).all() and (moved[~mask] == 0).all()
            assert (t["ceiling"][torch.from_numpy(ob.ceiling_raw == NO_CEILING)] == NO_CEILING).all()
    assert cur.read_state()[0] == int(g["count_at_cap"]) + 1 and cur.read_state()[1] == 0.25


def test_trigger_truth_table_and_one_count_per_eligible_step():
    ob = course(4)
    cur, t = make(ob, 6, "cpu")
    built = {k: v.clone() for k, v in t.items()}
    thr = cur.threshold
    for gc, rate, any_reset in ((6, thr, 1), (7, 1.0, 1), (12, 1.0, 0), (12, np.nextafter(thr, 0.0), 1), (-5, 1.0, 1)):
        twin_step(cur, gc, rate, any_reset)
        assert cur.read_state() == (0, 0.0, 0.0, -1), (gc, rate, any_reset)
        assert all(torch.equal(t[k], built[k]) for k in t)
    twin_step(cur, 12, np.nextafter(thr, 1.0))
    assert cur.read_state() == (1, 0.01, 0.01, 12)
    assert not torch.equal(t["height"], built["height"]) and torch.equal(t["height"], t["scan"])
    for gc in range(13, 18):                                   # ineligible steps in between: nothing moves
        twin_step(cur, gc, 1.0)
    assert cur.read_state()[0] == 1
    twin_step(cur, 18, 1.0)
    assert cur.read_state()[0] == 2 and cur.read_state()[3] == 18
    # the offset turns the step counter's twin into global_counter
    cur.set_offset(3)
    twin_step(cur, 24, 1.0)
    assert cur.read_state()[0] == 2
    twin_step(cur, 27, 1.0)
    assert cur.read_state() == (3, 0.03, 0.03, 24)


def test_count_goes_on_past_the_cap_with_clamped_biases():
    ob = course(4)
    cur, t = make(ob, 2, "cpu")
    cur.state[0] = cur.last - 1
    twin_step(cur, 2, 1.0)
    at_cap = {k: v.clone() for k, v in t.items()}
    assert cur.read_state()[:3] == (cur.last, 0.25, 0.25)
    for i in range(1, 4):
        twin_step(cur, 2 + 2 * i, 1.0)
        assert cur.read_state()[:3] == (cur.last + i, 0.25, 0.25)
        assert all(torch.equal(t[k], at_cap[k]) for k in t)
    built = torch.from_numpy(ob.height_field_raw)
    assert int((t["height"] - built).max()) == 50 and int((t["height"] - built).min()) == 0          # 0.25 m of 5 mm samples


def test_increment_tables_are_the_float64_expression():
    """a (curr_step, vertical_scale) pair, found by the generator's search, at which fp32 truncates to another integer"""
    g = np.load(GOLD)
    cs, vs, count = float(g["fp_curr_step"]), float(g["fp_vertical_scale"]), int(g["fp_count"])
    r = [float(v) for v in g["fp_max_range"]]
    inc, bias = oc.increment_tables(cs, vs, r, r)
    assert inc.dtype == np.int32 and bias.dtype == np.float64
    assert np.array_equal(inc[:, 0], g["fp_increments"]) and np.array_equal(inc[:, 1], g["fp_increments"])
    b32 = np.float32(np.float32(bias[count, 0]) / np.float32(vs))
    assert int(b32) != int(inc[count, 0])                      # the case is live: fp32 arithmetic would have got it wrong
    assert bias[-1, 0] == bias[-2, 0] == r[1] - r[0] and bias[-3, 0] < bias[-2, 0]
    # the default configuration: 26 raises to the cap, one row past it
    c = Go2AgilityCfg.obstacle
    inc, bias = oc.increment_tables(c.curr_step, c.vertical_scale, c.bar_jump_max_range, c.tire_jump_max_range)
    assert inc.shape == (27, 2) and [int(min(k * c.curr_step, 0.3 - 0.05) / c.vertical_scale) for k in range(27)] == inc[:, 0].tolist()


def test_library_exports_the_entry_point_and_capi_binds_it():
    import __graft_entry__ as g
    g.build()
    lib = _capi.load_library()
    assert "tsc_obstacle_curriculum" in _capi.EXTENSION_SYMBOLS and "tsc_obstacle_curriculum" not in _capi.ABI_SYMBOLS
    f = lib.qa_tsc_obstacle_curriculum
    assert f.restype == C.c_int and len(f.argtypes) == 2
    assert f(None, None) == -1                                                     # QA_E_ARG, nothing touches the device
    a = _capi.QaTscObstCurr()
    assert f(C.byref(a), None) == -1 and b"qa_tsc_obstacle_curriculum" in lib.qa_last_error()
    text = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "qa_tsc_curriculum.h")).read()
    assert "qa_tsc_obstacle_curriculum(" in text and "legged_robot.py:917-957" in text
    assert "qa_tsc_obstacle_curriculum" not in open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "qa_sim.h")).read()


def _stagger(env):
    """episode clocks 0, 1, 2, 0, ... so that somebody times out on every step of a 2-step episode"""
    env.episode_length_buf = (torch.arange(env.num_envs) % 3).to(env.episode_length_buf)


def test_env_raises_on_the_schedule_and_not_in_the_constructor():
    """the oracle-backend env (the torch twin inside `_reset`): a threshold below every rate would raise at global_counter 0 if the
    constructor's reset counted; afterwards one raise per period, every map and the goals follow, and a rate at the threshold stops it"""
    from tests.test_tsc_course_env import cpu_env
    env = cpu_env(4, seed=11, obstacle__curriculum=True, obstacle__curr_threshold=-1.0, env__episode_length_s=0.04)
    assert env.obstacle_curriculum_armed and env.max_episode_length == 2 and env._oc.period == 4
    assert (env.obst_curr_count, env.bar_jump_bias, env.tire_jump_bias) == (0, 0.0, 0.0)
    ob = env.obstacle
    assert np.array_equal(env.sim.t["HEIGHT_SAMPLES"].numpy(), ob.height_field_raw)
    _stagger(env)
    env.sync_reset_ids = False
    hist = torch.zeros(4, 8, 19)
    for k in range(1, 10):
        env.set_commands(torch.zeros(4, 19))
        env.step(torch.zeros(4, 12), hist)
        assert env.global_counter == k and env.obst_curr_count == k // 4, k
    inc = int(0.02 / 0.005)
    bar, tyre = torch.from_numpy(ob.bar_jump_mask), torch.from_numpy(ob.tire_jump_mask)
    for m in (env.sim.t["HEIGHT_SAMPLES"], env.bk.height_samples, env.height_samples):
        d = m - torch.from_numpy(ob.height_field_raw)
        assert (d[bar] == inc).all() and (d[tyre] == inc).all() and (d[~(bar | tyre)] == 0).all()
    d = env.sim.t["CEILING_SAMPLES"] - torch.from_numpy(ob.ceiling_raw)
    tc = torch.from_numpy(ob.tire_ceiling_mask)
    assert (d[tc] == inc).all() and (d[~tc] == 0).all()
    g = torch.from_numpy(ob.flat_goals()).float()
    changed = env.env_goals != g
    assert int(changed.sum()) >= 4 and torch.allclose(env.env_goals[changed], g[changed] + 0.02, atol=1e-6)
    assert env.bar_jump_bias == 0.02 and env.tire_jump_bias == 0.02
    # the current goals were gathered from the raised goals
    idx = env.cur_goal_idx.clamp(0, 25)[:, None, None].expand(-1, 1, 3)
    assert torch.equal(env.cur_goals, env.env_goals.gather(1, idx).squeeze(1))
    # success_rate is the device scalar too: at the threshold nothing moves any more
    env._oc.threshold = 0.8
    env.success_rate = 0.8
    for k in range(10, 14):
        env.step(torch.zeros(4, 12), hist)
    assert env.obst_curr_count == 2
    env.success_rate = 0.81
    for k in range(14, 17):
        env.step(torch.zeros(4, 12), hist)
    assert env.obst_curr_count == 3 and env._oc.read_state()[3] == 16


def test_camera_env_does_not_arm_and_learn_vision_disarms(capsys, tmp_path):
    from tests.test_tsc_course_env import cpu_env
    cam = cpu_env(4, seed=11, obstacle__curriculum=True, depth__use_camera=True)
    assert "obstacle curriculum: not armed" in capsys.readouterr().out
    assert not cam.obstacle_curriculum_armed and cam._oc is None and cam.obst_curr_count == 0 and cam.bar_jump_bias == 0
    cam.success_rate = 1.0                                     # still an attribute the runner may set
    assert cam.success_rate == 1.0
    off = cpu_env(4, seed=11)
    assert not off.obstacle_curriculum_armed and off._oc is None
    # learn_vision clears cfg.obstacle.curriculum on entry (on_policy_runner.py, as the reference's): an armed env stops raising
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    env = cpu_env(4, seed=11, obstacle__curriculum=True, obstacle__curr_threshold=-1.0, env__episode_length_s=0.04)
    tcfg = class_to_dict(Go2AgilityCfgPPO())
    tcfg["runner"]["num_steps_per_env"] = 4
    runner = OnPolicyRunner(env, tcfg, log_dir=None, device="cpu")
    assert env.obstacle_curriculum_armed
    try:
        runner.learn_vision(0)
    except Exception:                                          # a teacher's runner has no depth student: the flags are cleared before it is needed
        pass
    assert env.cfg.obstacle.curriculum is False and not env.obstacle_curriculum_armed
    _stagger(env)
    for _ in range(5):
        env.step(torch.zeros(4, 12), torch.zeros(4, 8, 19))
    assert env.global_counter == 5 and env.obst_curr_count == 0
    assert np.array_equal(env.sim.t["HEIGHT_SAMPLES"].numpy(), env.obstacle.height_field_raw)


def _rate_worker(rank, world, port, q):
    import types
    import torch.distributed as dist
    from tests.test_distributed_cpu import _init
    _init(rank, world, port)
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    window = [1.0, 1.0, 1.0, 0.0] if rank == 0 else [0.0] * 6 + [1.0] * 2          # local means 0.75 and 0.25, job mean 5 / 12
    rate = OnPolicyRunner._job_success_rate(types.SimpleNamespace(device="cpu"), window)
    empty = OnPolicyRunner._job_success_rate(types.SimpleNamespace(device="cpu"), [])
    q.put((rank, rate, empty))
    dist.destroy_process_group()


def test_data_parallel_ranks_share_one_success_rate():
    import torch.multiprocessing as mp
    from tests.test_distributed_cpu import _free_port
    ctx = mp.get_context("spawn"); q = ctx.Queue(); port = _free_port()
    ps = [ctx.Process(target=_rate_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    out = sorted([q.get(timeout=120) for _ in ps], key=lambda t: t[0])
    [p.join(60) for p in ps]
    assert out[0][1] == out[1][1] == 5.0 / 12.0
    assert out[0][2] is None and out[1][2] is None


# ------------------------------------------------------------------ GPU
SEQUENCE = ((1, 1.0, 1), (6, 1.0, 1), (7, 1.0, 1), (12, 0.5, 1), (12, 1.0, 0), (12, 1.0, 1), (13, 1.0, 1), (18, 0.8, 1), (18, 0.9, 1), (24, 1.0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 9])
def test_kernel_equals_twin_bit_for_bit(n):
    """(global_counter, success rate, any_reset) over eligible and ineligible steps; 5 envs leave a grid row of the course partly empty.
    After every step: both height maps in full, the ceiling field, the goals and the state record"""
    ob = course(n)
    lib = _capi.load_library()
    kern, tk = make(ob, 6, "cuda")
    twin, tt = make(ob, 6, "cpu")
    kern.set_offset(2); twin.set_offset(2)
    step, any_reset = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    counts = []
    for gc, rate, flag in SEQUENCE + tuple((30 + 6 * i, 1.0, 1) for i in range(3)):
        if gc == 30:                                            # then up to and past the cap
            kern.state[0] = kern.last - 2; twin.state[0] = twin.last - 2
        step.fill_(gc + 2); any_reset.fill_(flag); kern.set_rate(rate)
        kern.launch(lib, step, any_reset, stream)
        torch.cuda.synchronize()
        twin.set_rate(rate)
        twin.update_torch(torch.tensor([gc + 2]), torch.tensor([flag], dtype=torch.uint8))
        for k in tt:
            assert torch.equal(tk[k].cpu(), tt[k]), (gc, k)
        assert torch.equal(kern.state.cpu(), twin.state), (gc, kern.state, twin.state)
        assert int(kern.ticket) == 0
        counts.append(kern.read_state()[0])
    assert counts[:10] == [0, 1, 1, 1, 1, 2, 2, 2, 3, 4] and counts[-1] == kern.last + 1
    built_c = torch.from_numpy(ob.ceiling_raw)
    tc = torch.from_numpy(ob.tire_ceiling_mask)
    c = tk["ceiling"].cpu()
    assert torch.equal(c[~tc], built_c[~tc]) and (c[tc] - built_c[tc] == 50).all() and (c[built_c == NO_CEILING] == NO_CEILING).all()
    # the launch geometry is a function of the list lengths only, and a single map is enough
    one, t1 = make(ob, 6, "cuda", two_maps=False)
    step.fill_(6); any_reset.fill_(1); one.set_rate(1.0)
    one.launch(lib, step, any_reset, stream)
    torch.cuda.synchronize()
    assert one.read_state()[0] == 1 and not torch.equal(t1["height"].cpu(), torch.from_numpy(ob.height_field_raw))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 9])
def test_hip_env_matches_oracle_env_across_a_raise(n):
    """the protocol of tests/test_tsc_course_env.py::test_two_level_pipeline_matches_oracle_on_gpu (state re-synchronised every step,
    tolerances of tests/parity_tol.py) with the curriculum armed on both sides: a 2-step episode makes the period 4 steps"""
    from tests.test_hip_parity import BUDGET, check_flips, env_mismatch
    from tests.test_tsc_course_env import _gpu_pair
    env_g, env_o = _gpu_pair(n, 11, obstacle__curriculum=True, env__episode_length_s=0.04)
    assert env_g.obstacle_curriculum_armed and env_o.obstacle_curriculum_armed and env_g._glue_kernels() and not env_o._glue_kernels()
    _stagger(env_g); _stagger(env_o)
    env_g.success_rate = env_o.success_rate = 0.9
    env_o.sync_reset_ids = env_g.sync_reset_ids = False
    hist = torch.zeros(n, 8, 19)
    names = ("ROOT_STATES", "DOF_STATE", "CONTACT_FORCES", "RIGID_BODY_POS", "TORQUES", "ACTIONS", "LAST_DOF_VEL")
    flips, steps = 0, 9
    for k in range(1, steps + 1):
        env_g.sim.arena.copy_(torch.from_numpy(env_o.sim.o.arena.copy()).cuda())
        for name in ("commands", "latent_eps", "latent_c", "episode_length_buf", "cur_goal_idx", "reach_goal_timer", "last_contacts", "cur_goals",
                     "next_goals", "episode_sums_buf", "obs_history_buf", "delta_yaw", "delta_next_yaw", "obs_bbc_buf", "obs_disc_buf"):
            getattr(env_g.bk, name).copy_(getattr(env_o.bk, name).cuda())
        a = torch.zeros(n, 19)
        env_o.bk.set_commands(a, None); env_g.bk.set_commands(a.cuda(), None)
        env_o.step(torch.zeros(n, 12), hist); env_g.step(torch.zeros(n, 12).cuda(), hist.cuda())
        torch.cuda.synchronize()
        assert env_g.global_counter == env_o.global_counter == k and int(env_g._step_dev) == int(env_o._step_dev) == k + 1
        assert env_g._oc.read_state() == env_o._oc.read_state() and env_g.obst_curr_count == k // 4, k
        # every holder of the course, bit for bit
        assert torch.equal(env_g.sim.t["HEIGHT_SAMPLES"].cpu(), env_o.sim.t["HEIGHT_SAMPLES"]) and torch.equal(env_g.bk.height_samples.cpu(), env_o.bk.height_samples)
        assert torch.equal(env_g.sim.t["CEILING_SAMPLES"].cpu(), env_o.sim.t["CEILING_SAMPLES"])
        assert torch.equal(env_g.env_goals.cpu(), env_o.env_goals)
        bad = np.zeros(n, bool)
        for name in names:
            bad |= env_mismatch(name, env_g.sim.t[name].cpu().numpy(), env_o.sim.t[name].numpy(), n)
        ok = ~bad
        flips += int(bad.sum())
        for name in ("reset_buf", "time_out_buf", "episode_length_buf", "cur_goal_idx"):
            assert torch.equal(getattr(env_g.bk, name).cpu()[ok], getattr(env_o.bk, name)[ok]), (k, name)
        assert torch.equal(env_g.bk.cur_goals.cpu()[ok], env_o.bk.cur_goals[ok])
        assert torch.allclose(env_g.bk.rew_buf.cpu()[ok], env_o.bk.rew_buf[ok], atol=2e-4, rtol=1e-3)
        for name in ("obs_buf", "obs_bbc_buf", "obs_disc_buf"):
            g, o = getattr(env_g.bk, name).cpu()[ok], getattr(env_o.bk, name)[ok]
            assert torch.allclose(g, o, atol=3e-3, rtol=1e-3), (k, name, float((g - o).abs().max()))
        assert torch.equal(env_g.bk.measured_heights.cpu()[ok], env_o.bk.measured_heights[ok])
    assert env_g.obst_curr_count == 2 and env_g.bar_jump_bias == 0.02
    assert not torch.equal(env_g.sim.t["HEIGHT_SAMPLES"].cpu(), torch.from_numpy(env_g.obstacle.height_field_raw))
    check_flips(f"course_curriculum_{n}", flips, steps * n, BUDGET["course"])


def _teacher(n, log_dir, **flags):
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    from tests.test_tsc_course_env import make_cfg
    cfg = make_cfg(n, 1, obstacle__curriculum=True, env__episode_length_s=0.1, obstacle__randomize_start=True, **flags)
    env = lr.LeggedRobot(cfg, sim_device="cuda:0")
    return env, OnPolicyRunner(env, class_to_dict(Go2AgilityCfgPPO()), log_dir=log_dir, device="cuda:0")


@pytest.mark.gpu
def test_recorded_rollout_equals_eager_rollout_across_a_raise():
    """128 envs (the smallest the task-level tree's recorded-rollout tests use), 5-step episodes: the period is 10 of a rollout's 24 steps.
    Iterations 0 and 1 are the eager warm-ups of the two actor variants, 2 records and replays with the success rate over the threshold (it
    raises three times inside the replay), 3 replays again with the rate back under it (it must not raise again)."""
    out = {}
    for mode in ("recorded", "eager"):
        torch.manual_seed(0)
        env, runner = _teacher(128, None)
        runner.use_rollout_graph = mode == "recorded"
        assert env._oc.period == 10
        snaps = []
        for it, rate in enumerate((0.0, 0.0, 0.9, 0.5)):
            env.success_rate = rate
            runner.learn(1, init_at_random_ep_len=(it == 0))
            torch.cuda.synchronize()
            snaps.append(dict(height=env.sim.t["HEIGHT_SAMPLES"].clone(), scan=env.bk.height_samples.clone(), ceiling=env.sim.t["CEILING_SAMPLES"].clone(),
                              goals=env.env_goals.clone(), state=env._oc.state.clone(), obs=runner.alg.storage.observations.clone(),
                              root=env.root_states.clone(), cur_goals=env.cur_goals.clone()))
            assert env.global_counter == 24 * (it + 1) and int(env._step_dev) == env.common_step_counter == 1 + 24 * (it + 1)
        if mode == "recorded":
            assert any(isinstance(v, tuple) for v in runner._rollout_graphs.values())
        out[mode] = snaps
    for it in range(4):
        for k in out["eager"][it]:
            assert torch.equal(out["eager"][it][k], out["recorded"][it][k]), f"iteration {it}: `{k}` differs between the recorded and the eager rollout"
    r = out["recorded"]
    assert [int(s["state"][0]) for s in r] == [0, 0, 3, 3]                         # global_counter 50, 60 and 70 fall into the third rollout
    assert int(r[2]["state"][3]) == 70
    assert torch.equal(r[0]["height"], r[1]["height"]) and not torch.equal(r[1]["height"], r[2]["height"]) and torch.equal(r[2]["height"], r[3]["height"])
    assert not torch.equal(r[1]["goals"], r[2]["goals"]) and not torch.equal(r[1]["ceiling"], r[2]["ceiling"])


@pytest.mark.gpu
def test_logged_run_reports_the_bias(tmp_path):
    """learn_RL with a log directory and a threshold every rate passes: the runner writes the reference's key, and the tyre's"""
    class Rec:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, value, step):
            self.rows.append((tag, float(value), int(step)))
    torch.manual_seed(0)
    env, runner = _teacher(128, str(tmp_path), obstacle__curr_threshold=-1.0)
    runner.writer = Rec()
    runner.learn(3, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    bar = [v for t, v, _ in runner.writer.rows if t == "Curr/bar_jump_bias"]
    tyre = [v for t, v, _ in runner.writer.rows if t == "Curr/tire_jump_bias"]
    assert len(bar) == len(tyre) == 3 and bar == tyre
    assert bar == [0.02, 0.04, 0.07]                           # global_counter 10, 20 | 30, 40 | 50, 60, 70
    assert env.obst_curr_count == 7 and env.bar_jump_bias == 0.07
