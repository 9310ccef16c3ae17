"""-m gpu: the calf-against-neighbouring-hip self-collision class of the HIP env kernels (qa_set_self_collision_hips, include/qa_sim_selfcol.h,
DESIGN.md 3.4).  The CPU oracle has no twin of it, so these are known-answer tests on the kernels themselves: a front leg driven into the rear hip
of its side stops at the surfaces (and passes through with the feature off), the contact is an internal force reported on one calf and one hip with
opposite signs, a hip force above 1 N ends the episode on that step, ordinary gaits never touch and the feature being on changes nothing for them,
a wavefront that holds touching and non-touching envs leaves the latter alone, and a recorded rollout equals the eager one.

Gaps are computed in float64 from DOF_STATE by tests/selfcol_hips_ref.py, never from anything the kernel exports.  QA_ENV_HELPERS is read once per
process, so the scenarios that are to run with and without helper wavefronts run in two child processes (tests/test_env_helpers.py's pattern);
one child runs all of them and the tests share its result."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import selfcol_hips_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALF, HIP, FOOT = [5 + 4 * l for l in range(4)], [3 + 4 * l for l in range(4)], [6 + 4 * l for l in range(4)]
# front legs swept back with the knee half opened: found on the CPU with the float64 FK on the oracle's trajectory (without the rows the
# front calves go 24 mm into the rear hips and come to rest 16 mm inside, at thigh 2.15 rad / calf -1.3 rad); the rear legs hold the default
# pose.  (A harder drive, e.g. calf action 4 = a target beyond the knee's stop, leaves the explicit PD loop of a folded leg in a
# velocity-clamped limit cycle with or without any contact row -- the oracle shows it too -- and the clamp is not momentum-neutral.)
DRIVE = np.array([0.0, 5.0, 2.0, 0.0, 5.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)
SLOP = -0.004            # the calf-calf test's bound (tests/test_self_collision.py): 4 sweeps, 5 ms substeps, the same depenetration cap
PAIRS = [(0, 2), (1, 3)]  # (calf leg, hip leg) of the two rows

CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.oracle_lib import OracleSim, go2_cfg
from tests.test_self_collision import CROSS, FOLD
from tests.test_selfcol_hips import DRIVE
from quadrupedal_agility_amd.sim import QaSim
out = sys.argv[1]
res = {}

def free_robots(n, hips, gravity=-9.81):
    # tests/test_self_collision.py::_free_robot for n envs, on the GPU
    q = go2_cfg(n, randomize_base_mass=0, randomize_base_com=0, randomize_motor=0, randomize_friction=0, gravity_z=gravity, push_robots=0, add_noise=0, self_collision=1)
    o = OracleSim(q); o.reset_all()
    o.t["ROOT_STATES"][:] = [0, 0, 40.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    o.t["DOF_STATE"][:, :, 0] = [0, 0.9, -1.8] * 4; o.t["DOF_STATE"][:, :, 1] = 0
    o.t["EPISODE_LENGTH"][:] = 5
    return q, o

def handle(q, o, hips):
    h = QaSim(q, "cuda:0")
    h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
    if hips:
        h.set_self_collision_hips(True)
    return h

def finite(h):
    return all(bool(torch.isfinite(h.t[k]).all()) for k in ("ROOT_STATES", "DOF_STATE", "CONTACT_FORCES", "RIGID_BODY_POS"))

# cases 1, 2: a constant action through physics_step (nothing resets)
for tag, act in (("drive", DRIVE), ("fold", FOLD)):
    for hips in (0, 1):
        q, o = free_robots(1, hips); h = handle(q, o, hips)
        a = torch.from_numpy(act[None]).cuda()
        dof, rb, ok = [], [], True
        for _ in range(50):
            h.physics_step(a); torch.cuda.synchronize()
            dof.append(h.t["DOF_STATE"][0, :, 0].cpu().numpy()); rb.append(h.t["RIGID_BODY_POS"][0].cpu().numpy()); ok = ok and finite(h)
        res[f"{tag}{hips}_dof"] = np.array(dof); res[f"{tag}{hips}_rb"] = np.array(rb); res[f"{tag}{hips}_finite"] = np.array(ok)

# case 3: zero gravity, no ground; the new class (DRIVE, on) and the calf-calf class (CROSS, off: the parent's behaviour) by the same procedure
for tag, act, hips in (("mom_hips", DRIVE, 1), ("mom_calves", CROSS, 0)):
    q, o = free_robots(1, hips, gravity=0.0)
    o.t["ROOT_STATES"][0, 7:13] = [0.3, -0.2, 0.1, 0.2, 0.1, -0.3]
    h = handle(q, o, hips)
    a = torch.from_numpy(act[None]).cuda()
    for _ in range(10):
        h.physics_step(a)
    torch.cuda.synchronize()
    res[tag + "_root0"] = h.t["ROOT_STATES"][0].cpu().numpy(); res[tag + "_dof0"] = h.t["DOF_STATE"][0].cpu().numpy()
    cf = []
    for _ in range(50):
        h.physics_step(a); torch.cuda.synchronize()
        cf.append(h.t["CONTACT_FORCES"][0].cpu().numpy())
    res[tag + "_cf"] = np.array(cf)
    res[tag + "_root1"] = h.t["ROOT_STATES"][0].cpu().numpy(); res[tag + "_dof1"] = h.t["DOF_STATE"][0].cpu().numpy()

# case 4: the same drive through step(): the fused step's own termination check
for hips in (0, 1):
    q, o = free_robots(1, hips); h = handle(q, o, hips)
    a = torch.from_numpy(DRIVE[None]).cuda()
    reset, tout, cf = [], [], []
    for _ in range(14):
        h.step(a); torch.cuda.synchronize()
        reset.append(int(h.t["RESET"][0])); tout.append(int(h.t["TIME_OUT"][0])); cf.append(h.t["CONTACT_FORCES"][0].cpu().numpy())
    res[f"term{hips}_reset"] = np.array(reset); res[f"term{hips}_timeout"] = np.array(tout); res[f"term{hips}_cf"] = np.array(cf)

# case 6: one wavefront of 16 envs x 4 with touching and non-touching envs side by side
n = 64
rng = np.random.default_rng(4)
acts = [(rng.normal(0, 0.5, (n, 12))).astype(np.float32) for _ in range(20)]
for a in acts:
    a[::4] = DRIVE
for hips in (0, 1):
    q, o = free_robots(n, hips); h = handle(q, o, hips)
    dof = []
    for a in acts:
        h.physics_step(torch.from_numpy(a).cuda()); torch.cuda.synchronize()
        dof.append(h.t["DOF_STATE"][:, :, 0].cpu().numpy())
    res[f"mixed{hips}_dof"] = np.array(dof)
    for k, v in h.t.items():
        if v.dim() >= 1 and v.shape[0] == n:
            res[f"mixed{hips}_T_{k}"] = v.cpu().numpy()
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the scenarios above, once per helper setting"""
    d = tmp_path_factory.mktemp("selfcol_hips")
    outs = {}
    for mode in ("0", "1"):
        out = str(d / f"helpers{mode}.npz")
        subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], check=True, env=dict(os.environ, QA_ENV_HELPERS=mode), timeout=600)
        outs[mode] = np.load(out)
    return outs


def calf_calf_gaps(rb):
    """(steps, 19, 3) body positions -> (steps, 4) gaps of the calf-calf pairs, by the closed form"""
    rb = rb.astype(np.float64)
    out = []
    for a, b in [(0, 1), (2, 3), (0, 2), (1, 3)]:
        d, s, t = ref.seg_seg(rb[:, CALF[a]], rb[:, FOOT[a]], rb[:, CALF[b]], rb[:, FOOT[b]])
        out.append(d - (0.013 + 0.009 * s) - (0.013 + 0.009 * t))
    return np.stack(out, -1)


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_a_leg_driven_into_a_hip_stops_at_the_surfaces(runs, helpers):
    r = runs[helpers]
    off, on = ref.all_gaps(r["drive0_dof"]), ref.all_gaps(r["drive1_dof"])
    print("calf-hip gaps (m), feature off / on, min over 50 steps:", off.min(0), on.min(0))
    for k in range(2):                                          # the two front-calf / rear-hip relations
        assert off[:, k].min() < -0.010, (k, off[:, k].min())   # without the rows the calf passes through the hip: the pose does reach it
        assert on[:, k].min() > SLOP, (k, on[:, k].min())       # with them it stops at the surfaces
    assert bool(r["drive1_finite"]) and bool(r["drive0_finite"])
    assert np.isfinite(r["drive1_dof"]).all()


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_front_back_fold_keeps_every_front_rear_gap(runs, helpers):
    """FOLD (front legs back, rear legs forward): every calf-hip gap of the front / rear relations -- both orderings -- and the calf-calf gaps"""
    r = runs[helpers]
    ch = ref.all_gaps(r["fold1_dof"])
    cc = calf_calf_gaps(r["fold1_rb"])
    print("FOLD, feature on: calf-hip min", ch.min(0), "calf-calf min", cc.min(0))
    assert ch.min() > SLOP and cc.min() > SLOP
    assert bool(r["fold1_finite"])
    assert calf_calf_gaps(r["fold0_rb"])[:, 2:].min() < 0.01    # the front / rear calves do meet in this pose (the calf-calf rows are active beside the new one)


def _momentum(lib, root, dof):
    from tests.test_oracle_physics import bodies, quat_to_mat
    root = root.astype(np.float64); R = quat_to_mat(root[3:7])
    ub = np.concatenate([R.T @ root[10:13], R.T @ root[7:10]])
    com, vel, omg, mass, I = bodies(lib, dof[:, 0].copy(), dof[:, 1].copy(), ub)
    p = sum(mass[b] * (R @ vel[b]) for b in range(13))
    c = sum(mass[b] * (R @ com[b]) for b in range(13)) / mass.sum()
    L = sum(mass[b] * np.cross(R @ com[b] - c, R @ vel[b]) + R @ (I[b] @ omg[b]) for b in range(13))
    return p, L


def test_the_contact_is_an_internal_force(runs, oracle_lib):
    """zero gravity, no ground, 10 settling steps, then 50: opposite forces on one calf and one hip, nothing elsewhere, momentum unchanged.
    The momentum tolerance is MEASURED: the drift of the calf-calf class (CROSS, feature off -- the parent's behaviour) by the same procedure on
    the same kernels, times two (fp32 rounding differs by pose).  profiles/self_collision_hips_kats.json records both."""
    r = runs["0"]
    cf = r["mom_hips_cf"]
    in_pair = sorted([CALF[a] for a, _ in PAIRS] + [HIP[b] for _, b in PAIRS])
    for step in cf:
        for a, b in PAIRS:
            assert np.allclose(step[CALF[a]], -step[HIP[b]], atol=1e-4), (step[CALF[a]], step[HIP[b]])
        assert np.abs(np.delete(step, in_pair, axis=0)).max() == 0.0
    peak = float(np.linalg.norm(cf[:, HIP], axis=-1).max())
    assert peak > 5.0, peak
    drift = {}
    for tag in ("mom_hips", "mom_calves"):
        p0, L0 = _momentum(oracle_lib, r[tag + "_root0"], r[tag + "_dof0"]); p1, L1 = _momentum(oracle_lib, r[tag + "_root1"], r[tag + "_dof1"])
        drift[tag] = (float(np.abs(p1 - p0).max()), float(np.abs(L1 - L0).max()))
    assert float(np.abs(r["mom_calves_cf"][:, CALF]).max()) > 5.0          # the yardstick run did have its legs in contact
    print("momentum drift over 50 steps (linear kg m/s, angular kg m^2/s): calf-hip", drift["mom_hips"], "calf-calf", drift["mom_calves"], "peak hip force (N)", peak)
    assert drift["mom_hips"][0] <= 2 * drift["mom_calves"][0] and drift["mom_hips"][1] <= 2 * drift["mom_calves"][1], drift


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_a_hip_contact_ends_the_episode_on_that_step(runs, helpers):
    r = runs[helpers]
    on_reset, off_reset = r["term1_reset"], r["term0_reset"]
    hipf = np.linalg.norm(r["term1_cf"][:, HIP], axis=-1).max(axis=-1)           # (steps,) largest hip force
    first = int(np.argmax(hipf > 1.0))
    print("largest hip force per step (N):", np.round(hipf, 2), "RESET:", on_reset)
    assert hipf[first] > 1.0
    assert on_reset[first] == 1 and not on_reset[:first].any()                   # on the first step whose hip force exceeds 1 N, and not before
    assert not off_reset.any()                                                   # no other termination fires over these steps
    assert not r["term1_timeout"][:first + 1].any() and not r["term0_timeout"].any()
    assert np.linalg.norm(r["term0_cf"][:, HIP], axis=-1).max() == 0.0


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_mixed_wavefront_leaves_the_other_envs_alone(runs, helpers):
    r = runs[helpers]
    n = 64
    driven = np.arange(n) % 4 == 0
    names = [k[len("mixed0_T_"):] for k in r.files if k.startswith("mixed0_T_")]
    assert "DOF_STATE" in names and "ROOT_STATES" in names and "CONTACT_FORCES" in names
    for k in names:
        a, b = r["mixed0_T_" + k], r["mixed1_T_" + k]
        assert np.array_equal(a[~driven], b[~driven], equal_nan=True), k        # the wave-uniform votes do not leak into lanes whose pair is apart
    assert np.array_equal(r["mixed0_dof"][:, ~driven], r["mixed1_dof"][:, ~driven])
    on, off = ref.all_gaps(r["mixed1_dof"][:, driven]), ref.all_gaps(r["mixed0_dof"][:, driven])
    assert off[..., :2].min() < -0.010 and on[..., :2].min() > SLOP, (off[..., :2].min(), on[..., :2].min())
    assert ref.all_gaps(r["mixed1_dof"][:, ~driven]).min() > ref.CONTACT_OFFSET     # (and the random-action envs were indeed apart)


def _random_steps(h, n, steps, seed, record=None):
    import torch
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        h.step((torch.randn(n, 12, generator=g) * 0.5).cuda())
        if record is not None:
            record.append(h.t["DOF_STATE"][:, :, 0].cpu().numpy())
    torch.cuda.synchronize()


def test_off_is_off_and_ordinary_gaits_never_touch():
    """17 envs: the last (only) wavefront is partial.  40 random-action steps from reset_all() with the flag on and off: bit-identical arenas,
    and the smallest calf-hip gap stays above the contact offset"""
    import torch
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    n = 17
    arenas, dofs = [], []
    for hips in (True, False, None):
        h = QaSim(go2_cfg(n, seed=3, self_collision=1), "cuda:0")
        if hips is not None:
            h.set_self_collision_hips(hips)                # None: never called
        h.reset_all()
        rec = []
        _random_steps(h, n, 40, seed=8, record=rec)
        arenas.append(h.arena.clone()); dofs.append(np.array(rec))
    assert torch.equal(arenas[0], arenas[1]) and torch.equal(arenas[1], arenas[2])
    assert ref.all_gaps(dofs[0]).min() > ref.CONTACT_OFFSET, ref.all_gaps(dofs[0]).min()


def test_off_is_off_on_a_height_field_and_through_simulate():
    """the same on a height-field handle (tests/test_hip_parity.py::make_terrain_pair's config), with one qa_simulate at the end.  (Sloped contacts
    report their force through three multiply-adds; the instantiations with the rows spell out the fused form the others are compiled to --
    sloped_contact_force, csrc/qa_physics.h -- or the last bit of the foot forces would depend on the flag.)"""
    import torch
    from tests.test_hip_parity import make_terrain_pair, push_arena
    n = 17
    arenas = []
    for hips in (True, False):
        q, o, h = make_terrain_pair(n, 5, self_collision=1)
        o.reset_all()
        push_arena(o, h)
        if hips:
            h.set_self_collision_hips(True)
        rec = []
        _random_steps(h, n, 40, seed=9, record=rec)
        h.simulate(torch.zeros(n, 12, device="cuda")); torch.cuda.synchronize()
        arenas.append(h.arena.clone())
        assert ref.all_gaps(np.array(rec)).min() > ref.CONTACT_OFFSET
    assert torch.equal(arenas[0], arenas[1])


def test_setter_contract():
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    h = QaSim(go2_cfg(4, self_collision=0), "cuda:0")
    with pytest.raises(RuntimeError, match="self_collision"):
        h.set_self_collision_hips(True)                    # QA_E_ARG: the handle has no self-collision model
    h.set_self_collision_hips(False)
    h = QaSim(go2_cfg(4, self_collision=1), "cuda:0")
    h.set_self_collision_hips(True); h.set_self_collision_hips(False)


def test_recorded_rollout_equals_eager_rollout(monkeypatch):
    """small BBC rollouts with the flag on: hipGraph replays of the rollout against eager launches, the env arena bit for bit (the pattern of
    tests/test_terrain_curriculum.py::test_recorded_and_eager_rollouts_move_the_same_envs; the PPO update between the rollouts is not this
    feature's and has its own recorded-vs-eager tests)"""
    import torch
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    res = []
    for graph in ("1", "0"):
        monkeypatch.setenv("QA_ROLLOUT_GRAPH", graph)
        np.random.seed(0); torch.manual_seed(0)
        cfg = Go2LocomotionCfg(); cfg.env.num_envs = 64; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
        cfg.asset.qa_self_collision_hips = True
        t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = False
        args = get_args(["--device", "gpu"])
        env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
        assert env.self_collision_hips and env.sim.self_collision_hips
        runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=None)
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert (runner._graph is not None and not runner._graph_failed) == (graph == "1")
        res.append(env.sim.arena.clone())
    assert torch.equal(res[0], res[1])          # the env's whole state after two rollouts: observations, rewards, resets, contact forces
