"""-m gpu: recovery-pose resets and settable contact sets (include/qa_sim_reset.h) inside the kernels.

The fused step's recovery reset against the host restatement of tests/recovery_ref.py (itself pinned to the reference's outputs by
tests/test_recovery_init_cpu.py) on a plane, a height field and a height field with the terrain curriculum, for shard offsets 0 and 1000; the
per-step decision over twelve steps at seed 23; bit-identity on "no" steps, with the feature off and with the default masks; recorded ==
eager; lean == full; all of it again with and without helper wavefronts (child processes); the contact sets against THE REFERENCE'S outputs
under six list pairs (tests/golden/recovery_init.npz); 100 steps of tumbled spawns staying finite; the env class and the runner.
Tolerances: tests/test_mocap_reset.py's for poses, tests/test_extra_rewards.py's for REW; flags, counts and every bit-identity exact.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from quadrupedal_agility_amd import _capi, go2_limits
from tests import recovery_ref as rr
from tests.oracle_lib import go2_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
POSE_TOL = dict(atol=2e-6, rtol=1e-5)                 # tests/test_mocap_reset.py's
REW_TOL = dict(atol=1e-6, rtol=1e-5)                  # tests/test_extra_rewards.py's
SEED = 23                                             # decides steps 0..11 at p = 0.5 as 1,1,1,1,1,1,0,1,0,1,0,1 (tests/test_recovery_init_cpu.py)
NO_STEP, YES_STEP = 6, 5
SIZES = [64, 67]                                      # 67: a masked tail in the last wavefront


def plane_handle(n, seed=SEED, offset=0, **over):
    from quadrupedal_agility_amd.sim import QaSim
    q = go2_cfg(n, seed=seed, add_noise=0, push_robots=0, **over)
    q.env_id_offset = offset
    h = QaSim(q)
    h.reset_all()
    return q, h


def default_pose(q):
    return np.tile(np.array(list(q.default_dof_pos), np.float32)[:3], 4)


def expected_pose(q, h, ids, step):
    """the recovery pose of the (local) env ids at `step`, from host-computed uniforms and the origins the handle holds now"""
    ids = np.asarray(ids)
    u = rr.recovery_uniforms(int(q.seed), ids + int(q.env_id_offset), step)
    root, pos, vel = rr.recovery_pose(u, default_pose(q), list(q.init_pos), h.t["ENV_ORIGINS"].cpu().numpy()[ids])
    return root, np.stack([pos, vel], axis=-1)


def in_recovery_pose(q, h, ids, step):
    root, dof = expected_pose(q, h, ids, step)
    got_r, got_d = h.t["ROOT_STATES"].cpu().numpy()[ids], h.t["DOF_STATE"].cpu().numpy()[ids]
    return np.isclose(got_r, root, **POSE_TOL).all(1) & np.isclose(got_d, dof, **POSE_TOL).all((1, 2))


def step_resets(n, k):
    """the envs staged to time out in the k-th step of a run (k < 6): all inside ONE wavefront (16 envs), another wavefront from step to step, the
    last one -- at 67 envs the masked tail -- on step 2.  EPISODE_STATS is fed by float atomics, and the order in which different wavefronts reach
    it is not fixed; with a step's resets inside one wavefront whole arenas can be compared bit for bit."""
    last = (n - 1) // 16
    wave, second = [0, 1, last, 2, 0, 1][k], k >= 4
    if wave == last and n % 16:
        return [16 * last, n - 1]
    return [16 * wave + i + (1 if second else 0) for i in (1, 5, 9)]


def stagger(h, q, n, steps=6):
    for k in range(steps):
        h.t["EPISODE_LENGTH"][step_resets(n, k)] = int(q.max_episode_length) - k


# ---- reset mapping
def staged(n, variant, offset, prob):
    """a handle whose odd envs time out in the next step, on non-zero origins; `prob` set after the first reset_all"""
    import tests.test_terrain_curriculum as tc
    i = torch.arange(n, device="cuda")
    if variant == "plane":
        q, h = plane_handle(n, offset=offset)
        org = torch.stack([1.5 + 0.25 * i.float(), -2.0 + 0.125 * i.float(), torch.zeros(n, device="cuda")], dim=1)
        h.t["ENV_ORIGINS"].copy_(org)
        h.t["ROOT_STATES"][:, :2] += org[:, :2]
        ending = (i % 2) == 1
        h.t["EPISODE_LENGTH"].copy_(torch.where(ending, int(q.max_episode_length), 5))
        want_org = org
    else:
        q, h = tc.make_handle(n, seed=SEED, offset=offset, jitter=0.5)         # the default-pose path would jitter xy; the recovery pose has none
        tab = tc.table().cuda().contiguous()
        levels, types = (i % 3).contiguous(), ((i // 2) % tc.COLS).contiguous()
        ending = tc.stage(h, q, levels, types, tab, 0.05, 2.0, first=offset)
        h.t["ROOT_STATES"][:, 2] = tab[levels, types][:, 2] + float(q.init_pos[2])
        want_org = h.t["ENV_ORIGINS"].clone()
        if variant == "hfc":                                                    # 5 cm from the origin under a 2 m/s command: every ending env moves down
            want_org = torch.where(ending[:, None], tab[torch.clip(levels - 1, 0), types], want_org)
            h.set_terrain_curriculum(levels, types, tab, 8.0, tc.EPISODE_S)
            h._keep = (levels, types, tab)
    if prob is not None:
        h.set_recovery_init(prob)
    return q, h, ending, want_org


@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", ["plane", "hf", "hfc"])
def test_reset_mapping(variant, n, offset):
    step = 10
    assert bool(rr.recovery_steps(SEED, np.array([step]), 1.0)[0])
    q, h, ending, want_org = staged(n, variant, offset, 1.0)
    q0, h0, _, _ = staged(n, variant, offset, None)                             # the same step with the feature never set
    for x in (h, h0):
        x.global_step = step
        x.step(torch.zeros(n, 12, device="cuda"))
    torch.cuda.synchronize()
    reset = h.t["RESET"] != 0
    assert torch.equal(reset, ending) and torch.equal(h0.t["RESET"] != 0, ending)
    assert torch.equal(h.t["ENV_ORIGINS"], want_org)
    ids = reset.nonzero().flatten().cpu().numpy()
    root, dof = expected_pose(q, h, ids, step)
    got_r, got_d = h.t["ROOT_STATES"].cpu().numpy()[ids], h.t["DOF_STATE"].cpu().numpy()[ids]
    print(variant, n, offset, "max |root - host|", np.abs(got_r - root).max(), "max |dof - host|", np.abs(got_d - dof).max())
    assert np.allclose(got_r, root, **POSE_TOL) and np.allclose(got_d, dof, **POSE_TOL)
    assert np.array_equal(got_r[:, :3], root[:, :3])                             # init_pos + origin: one fp32 add, no jitter
    # the draws are those of the GLOBAL ids: another shard's envs get other poses
    if offset:
        local = rr.recovery_pose(rr.recovery_uniforms(SEED, ids, step), default_pose(q), list(q.init_pos), h.t["ENV_ORIGINS"].cpu().numpy()[ids])[0]
        assert not np.isclose(local[:, 3:], root[:, 3:], atol=1e-3).all(1).any()
    # the envs that did not reset are untouched by it, and everything a reset does besides the pose is what any reset does
    keep = ~reset
    for name in ("ROOT_STATES", "DOF_STATE", "OBS", "LAST_DOF_VEL"):
        assert torch.equal(h.t[name][keep], h0.t[name][keep]), name
    for name in ("COMMANDS", "LATENT_C", "LATENT_EPS", "EPISODE_LENGTH", "EPISODE_SUMS", "REW", "TIME_OUT", "LAST_ACTIONS", "ACTION_HISTORY", "OBS_DISC_TERM"):
        assert torch.equal(h.t[name], h0.t[name]), name
    assert torch.equal(h.t["LAST_ROOT_VEL"][reset], h.t["ROOT_STATES"][reset, 7:13])           # taken after the reset (:160)
    assert torch.equal(h.t["LAST_DOF_VEL"][reset], h.t["DOF_STATE"][reset][..., 1])            # likewise (:158)


# ---- decision
@pytest.mark.parametrize("n", SIZES)
def test_decision_follows_the_host_prediction(n):
    want = rr.recovery_steps(SEED, np.arange(12), 0.5)
    assert want.astype(int).tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1]
    q, h = plane_handle(n)
    h.set_recovery_init(0.5)
    for k in range(12):
        ids = (5 * k + np.arange(5)) % n
        ids[-1] = n - 1 if k % 2 else ids[-1]                                   # the wavefront's tail takes part
        h.t["EPISODE_LENGTH"][torch.from_numpy(ids).cuda()] = int(q.max_episode_length)
        h.global_step = k
        h.step(torch.zeros(n, 12, device="cuda"))
        torch.cuda.synchronize()
        assert (h.t["RESET"].cpu().numpy()[ids] != 0).all()
        tumbled = in_recovery_pose(q, h, ids, k)
        root, dof = h.t["ROOT_STATES"].cpu().numpy()[ids], h.t["DOF_STATE"].cpu().numpy()[ids]
        if want[k]:
            assert tumbled.all(), k
        else:                                                                   # the handle's default-pose path
            assert not tumbled.any() and np.array_equal(root[:, 3:7], np.tile([0, 0, 0, 1], (5, 1)).astype(np.float32)) and (dof[..., 1] == 0).all(), k


# ---- bit-identity when the decision is "no"
def mocap_handles(n):
    from quadrupedal_agility_amd.sim import QaSim
    from tests.test_mocap_reset import real_clip_table
    _, (frames, clips, first) = real_clip_table()
    hs = []
    for _ in range(2):
        q = go2_cfg(n, seed=SEED, add_noise=0, push_robots=0, reset_mode=1, num_mocap_frames=int(frames.shape[0]))
        h = QaSim(q)
        h.set_mocap(frames, clips, first)
        h.reset_all()
        hs.append((q, h))
    return hs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["default_pose", "mocap"])
def test_a_no_step_is_bit_identical_to_the_feature_off(mode, n):
    TAIL = step_resets(n, 2)                # one wavefront's resets (at 67 envs the masked tail)
    (q, on), (_, off) = mocap_handles(n) if mode == "mocap" else [plane_handle(n), plane_handle(n)]
    on.set_recovery_init(0.5)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):                                                          # a state in motion, on `off`; `on` starts from a copy of it
        off.step(torch.randn(n, 12, generator=g).cuda() * 0.6)
    off.t["EPISODE_LENGTH"][TAIL] = int(q.max_episode_length)
    on.arena.copy_(off.arena)
    start = on.arena.clone()
    act = torch.randn(n, 12, generator=g).cuda() * 0.6
    assert not rr.recovery_steps(SEED, np.array([NO_STEP]), 0.5)[0] and rr.recovery_steps(SEED, np.array([YES_STEP]), 0.5)[0]
    for h in (on, off):
        h.global_step = NO_STEP
        h.step(act)
    torch.cuda.synchronize()
    assert (on.t["RESET"][TAIL] != 0).all()
    assert torch.equal(on.arena, off.arena)
    if mode == "mocap":
        assert not (on.t["ROOT_STATES"][TAIL, 3:7] == torch.tensor([0.0, 0, 0, 1], device="cuda")).all()     # frames, not the default pose
    # ... and it is the decision that keeps them equal: from the same arena a "yes" step parts them
    for h in (on, off):
        h.arena.copy_(start)
        h.global_step = YES_STEP
        h.step(act)
    torch.cuda.synchronize()
    assert in_recovery_pose(q, on, TAIL, YES_STEP).all() and not in_recovery_pose(q, off, TAIL, YES_STEP).any()
    keep = on.t["RESET"] == 0
    assert torch.equal(on.t["ROOT_STATES"][keep], off.t["ROOT_STATES"][keep]) and torch.equal(on.t["OBS"][keep], off.t["OBS"][keep])


# ---- off and defaults
def _arena_after(n, mode, steps=3):
    from quadrupedal_agility_amd.sim import QaSim
    q = go2_cfg(n, seed=9, add_noise=0, push_robots=0)
    h = QaSim(q)
    if mode == "cleared":
        h.set_recovery_init(0.3); h.set_contact_sets(_capi.BODY_CLASS_BITS["calf"], 0)
        h.set_recovery_init(0.0); h.set_contact_sets(_capi.DEFAULT_TERMINATION_MASK, _capi.DEFAULT_PENALISED_MASK)
    elif mode == "zero":
        h.set_recovery_init(0.0)
    elif mode == "default_masks":
        h.set_contact_sets(_capi.DEFAULT_TERMINATION_MASK, _capi.DEFAULT_PENALISED_MASK)
    h.reset_all()
    g = torch.Generator().manual_seed(11)
    for k in range(steps):
        h.t["EPISODE_LENGTH"][step_resets(n, k)] = int(q.max_episode_length)      # one wavefront's: the arenas below are compared whole
        h.step(torch.randn(n, 12, generator=g).cuda() * 0.7)
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("n", SIZES)
def test_off_is_off_and_default_masks_change_nothing(n):
    never, cleared, zero, masks = (_arena_after(n, m) for m in ("never", "cleared", "zero", "default_masks"))
    assert torch.equal(never.arena, cleared.arena) and torch.equal(never.arena, zero.arena) and torch.equal(never.arena, masks.arena)
    assert float(never.t["REW"].abs().sum()) > 0
    assert (never.t["RESET"][step_resets(n, 2)] != 0).all() and float(never.t["EPISODE_STATS"].abs().sum()) > 0


def test_setters_refuse_bad_arguments():
    q, h = plane_handle(8)
    assert h.recovery_init_prob == 0.0 and h.contact_sets == (_capi.DEFAULT_TERMINATION_MASK, _capi.DEFAULT_PENALISED_MASK)
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"\[0, 1\]"):
            h.set_recovery_init(bad)
    for bad in ((32, 0), (0, 64), (1 << 31, 0)):
        with pytest.raises(RuntimeError, match="QA_BC"):
            h.set_contact_sets(*bad)
    h.set_recovery_init(1.0); h.set_contact_sets(31, 31); h.set_contact_sets(0, 0); h.set_recovery_init(0.0)
    h.debug_post_physics(0); torch.cuda.synchronize()
    # either reset_mode, plane and height field
    import tests.test_terrain_curriculum as tc
    _, hf = tc.make_handle(8)
    hf.set_recovery_init(0.2)
    (_, m), _ = mocap_handles(8)
    m.set_recovery_init(0.2)


# ---- variants of the step
@pytest.mark.parametrize("n", SIZES)
def test_recorded_step_equals_eager_step(n):
    from quadrupedal_agility_amd.rsl_rl import recording
    hs = []
    for recorded in (False, True):
        q, h = plane_handle(n)
        h.set_recovery_init(0.5)                                     # before the recording: the launch arguments carry it
        h.set_contact_sets(_capi.BODY_CLASS_BITS["hip"], 13)
        ctr = torch.full((1,), 4, dtype=torch.int64, device="cuda")  # steps 4..7: yes, yes, no, yes
        act = (torch.randn(n, 12, generator=torch.Generator().manual_seed(13)) * 0.7).cuda()
        stagger(h, q, n, steps=4)
        h.step_dev(act, 0, ctr)                                      # one eager step first (warm-up of the recorded handle too)
        torch.cuda.synchronize()
        mid = None
        for _ in range(3):
            if recorded and mid is None:
                graph, _ = recording.record(lambda: h.step_dev(act, 0, ctr))
            graph.replay() if recorded else h.step_dev(act, 0, ctr)
            torch.cuda.synchronize()
            if int(ctr) == 7:                                        # after step 6, a "no": the handle's default pose
                mid = h.t["ROOT_STATES"][step_resets(n, 2), 3:7].clone()
        assert int(ctr) == 8
        hs.append((h, mid))
    (a, mid_a), (b, mid_b) = hs
    assert torch.equal(a.arena, b.arena) and torch.equal(mid_a, mid_b)
    assert torch.equal(mid_a, torch.tensor([0.0, 0, 0, 1], device="cuda").repeat(len(mid_a), 1))
    ids = step_resets(n, 3)
    assert (a.t["RESET"][ids] != 0).all() and in_recovery_pose(q, a, ids, 7).all() and float(a.t["EPISODE_STATS"].abs().sum()) > 0      # step 7: yes


LEAN_KEEPS = ("REW", "RESET", "TIME_OUT", "EPISODE_SUMS", "LAST_CONTACTS", "OBS", "ROOT_STATES", "DOF_STATE", "COMMANDS", "EPISODE_LENGTH")


def _rollout(variant, lean, n, steps=6):
    if variant == "plane":
        q, h = plane_handle(n)
    else:
        import tests.test_terrain_curriculum as tc
        q, h = tc.make_handle(n, seed=SEED)
    h.set_recovery_init(0.5)
    h.set_contact_sets(_capi.BODY_CLASS_BITS["hip"] | _capi.BODY_CLASS_BITS["calf"], 31)
    h.set_lean_exports(lean)
    stagger(h, q, n)
    g = torch.Generator().manual_seed(17)
    trace, tumbled = [], 0
    for k in range(steps):
        h.global_step = 3 + k                                        # steps 3..8: yes, yes, yes, no, yes, no
        h.step(torch.randn(n, 12, generator=g).cuda() * 0.8)
        torch.cuda.synchronize()
        trace.append({name: h.t[name].clone() for name in LEAN_KEEPS})
        ids = step_resets(n, k)
        assert (h.t["RESET"][ids] != 0).all()
        tumbled += int(in_recovery_pose(q, h, ids, 3 + k).sum())
    assert tumbled == sum(len(step_resets(n, k)) for k in (0, 1, 2, 4))          # the four "yes" steps
    return trace


@pytest.fixture(scope="module")
def full_rollouts():
    return {(v, n): _rollout(v, 0, n) for v in ("plane", "hf") for n in SIZES}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lean", [1, 3])
@pytest.mark.parametrize("variant", ["plane", "hf"])
def test_lean_steps_equal_the_full_step(full_rollouts, variant, lean, n):
    for a, b in zip(full_rollouts[(variant, n)], _rollout(variant, lean, n)):
        for name in a:
            assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_kernel_cases_with_and_without_helper_wavefronts(helpers):
    """QA_ENV_HELPERS is read once per process: the mapping, decision and lean cases again in a fresh child for each setting"""
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                          "test_reset_mapping or test_decision_follows_the_host_prediction or test_lean_steps_equal_the_full_step"],
                         cwd=ROOT, env=dict(os.environ, QA_ENV_HELPERS=helpers), capture_output=True, text=True, timeout=600)
    m = re.search(r"(\d+) passed", out.stdout)
    # 12 mapping cases + 2 decision cases + 8 lean cases, none skipped, none failed
    assert out.returncode == 0 and m and int(m.group(1)) == 22 and "skipped" not in out.stdout and "failed" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ---- contact sets against the reference
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "recovery_init.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def arena_gold():
    return np.load(os.path.join(GOLD, "extra_rewards.npz"), allow_pickle=False)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pair", range(6))
def test_contact_sets_match_the_reference(gold, arena_gold, pair, n):
    from tests.test_extra_rewards import load_case, tiled
    from tests.test_recovery_init_cpu import edited_forces
    from quadrupedal_agility_amd.sim import QaSim
    assert int(gold["num_pairs"]) == 6
    q = go2_cfg(n, seed=SEED, add_noise=0, push_robots=0)
    h = QaSim(q)
    h.set_extra_rewards(None)
    h.feet_air_time, h.extra_episode_sums = torch.zeros(n, 4, device="cuda"), torch.zeros(_capi.NUM_EXTRA_REWARDS, n, device="cuda")      # load_case fills them
    step = load_case(h, arena_gold, n)
    h.t["CONTACT_FORCES"].copy_(torch.from_numpy(tiled(edited_forces(gold), n)))
    term, pen = ([str(s) for s in gold[f"pair{pair}_terminate_on"]], [str(s) for s in gold[f"pair{pair}_penalize_on"]])
    h.set_contact_sets(rr.class_mask(term), rr.class_mask(pen))
    sums0 = h.t["EPISODE_SUMS"].clone()
    h.debug_post_physics(step)
    torch.cuda.synchronize()
    ref = lambda k: tiled(gold[f"pair{pair}_{k}"], n)
    rew = h.t["REW"].cpu().numpy()
    print(pair, term, pen, n, "max |REW - ref|", np.abs(rew - ref("rew")).max())
    assert np.array_equal(h.t["RESET"].cpu().numpy() != 0, ref("reset")) and np.array_equal(h.t["TIME_OUT"].cpu().numpy() != 0, ref("time_out"))
    assert np.allclose(rew, ref("rew"), **REW_TOL)
    # the collision term on its own: the running sum of the envs that did not reset moved by count x scale
    c = _capi.REWARD_NAMES.index("collision")
    keep = ~ref("reset")
    moved = (h.t["EPISODE_SUMS"][c] - sums0[c]).cpu().numpy()[keep]
    assert np.allclose(moved, ref("collision")[keep] * np.float32(q.reward_scale_dt[c]), atol=1e-6, rtol=1e-5)


# ---- tumbled spawns are inside the model
def test_tumbled_spawns_stay_finite_for_100_steps():
    n = 64
    q, h = plane_handle(n, seed=31)
    h.set_recovery_init(1.0)
    h.set_contact_sets(0, _capi.DEFAULT_PENALISED_MASK)              # no contact ends an episode: every env lives through all 100 steps
    assert int(q.max_episode_length) > 101
    h.global_step = 0
    h.reset_all()
    torch.cuda.synchronize()
    assert in_recovery_pose(q, h, np.arange(n), 0).all()
    lo = torch.tensor(go2_limits.DOF_POS_LOWER, dtype=torch.float32, device="cuda")
    hi = torch.tensor(go2_limits.DOF_POS_UPPER, dtype=torch.float32, device="cuda")
    outside0 = int(((h.t["DOF_STATE"][..., 0] < lo) | (h.t["DOF_STATE"][..., 0] > hi)).sum())
    inside_at, zmin, zmax = None, 1e9, -1e9
    zero = torch.zeros(n, 12, device="cuda")
    for k in range(100):
        h.step(zero)
        torch.cuda.synchronize()
        root, dof = h.t["ROOT_STATES"], h.t["DOF_STATE"]
        assert bool(torch.isfinite(root).all()) and bool(torch.isfinite(dof).all()) and bool(torch.isfinite(h.t["OBS"]).all()) and bool(torch.isfinite(h.t["REW"]).all()), k
        assert int((h.t["RESET"] != 0).sum()) == 0, k                # the non-finite guard (a time-out) never fires
        zmin, zmax = min(zmin, float(root[:, 2].min())), max(zmax, float(root[:, 2].max()))
        assert -0.05 <= float(root[:, 2].min()) and float(root[:, 2].max()) <= 1.0, k
        inside = bool(((dof[..., 0] >= lo) & (dof[..., 0] <= hi)).all())
        inside_at = (k + 1) if inside and inside_at is None else (inside_at if inside else None)
    print(f"tumbled spawns: {outside0} of {12 * n} joints start outside the URDF limits; every joint inside from step {inside_at} on; base height in [{zmin:.3f}, {zmax:.3f}] m")
    assert outside0 > 0


# ---- env and runner
def make_env(n=64, mocap=True):
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    np.random.seed(0); torch.manual_seed(0)
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"; cfg.seed = SEED
    cfg.env.mocap_state_init = mocap
    cfg.env.recovery_init_prob = 0.5
    cfg.asset.terminate_after_contacts_on = ["hip"]
    env, _ = task_registry.make_env("go2_locomotion", args=get_args(["--device", "gpu"]), env_cfg=cfg)
    return env


def test_runner_trains_with_recovery_resets(monkeypatch):
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    res, seen = [], 0
    for graph in ("1", "0"):
        monkeypatch.setenv("QA_ROLLOUT_GRAPH", graph)
        env = make_env()
        assert env.recovery_init_prob == 0.5 and env.sim.recovery_init_prob == 0.5 and env.sim.contact_sets == (2, 12) and env.contact_class_masks == (2, 12)
        if graph == "0":                                             # eager: look at every step's resets as they happen
            q, sim = env.qcfg, env.sim

            def watch(fn, step_of):
                def call(*a, **k):
                    nonlocal seen
                    step = step_of(*a)
                    fn(*a, **k)
                    torch.cuda.synchronize()
                    ids = (sim.t["RESET"] != 0).nonzero().flatten().cpu().numpy()
                    if len(ids):
                        hit = in_recovery_pose(q, sim, ids, step)
                        assert hit.all() if rr.recovery_steps(int(q.seed), np.array([step]), 0.5)[0] else not hit.any(), step
                        seen += int(hit.sum())
                return call
            monkeypatch.setattr(sim, "step", watch(sim.step, lambda *a: sim.global_step))
            monkeypatch.setattr(sim, "step_dev", watch(sim.step_dev, lambda a, d, ctr: int(ctr)))
        tcfg = Go2LocomotionCfgAlgo(); tcfg.runner.amp_enabled = False
        runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=get_args(["--device", "gpu"]), train_cfg=tcfg, log_root=None)
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert (runner._graph is not None and not runner._graph_failed) == (graph == "1")
        res.append({"sums": env.sim.t["EPISODE_SUMS"].clone(), "root": env.sim.t["ROOT_STATES"].clone()})
    a, b = res
    assert torch.equal(a["sums"], b["sums"]) and torch.equal(a["root"], b["root"])
    assert bool(torch.isfinite(a["root"]).all()) and seen >= 1


def test_env_without_mocap_init_reports_and_leaves_it_off(capsys):
    env = make_env(8, mocap=False)
    out = capsys.readouterr().out
    assert env.recovery_init_prob == 0.0 and env.sim.recovery_init_prob == 0.0
    assert len([l for l in out.splitlines() if "recovery_init_prob" in l]) == 1 and "mocap_state_init" in out
    assert env.sim.contact_sets == (2, 12)                            # the contact sets do not depend on it
