"""-m gpu: the calf-against-neighbouring-thigh self-collision class of the HIP env kernels (qa_set_self_collision_thighs, include/qa_sim_selfcol.h,
DESIGN.md 3.4).  The CPU oracle has no twin of it, so these are known-answer and bit-identity tests on the kernels themselves: a leg driven into the
thigh of the front / rear neighbour stops at the surfaces (and passes through at level 1), the contact is an internal force reported on one calf and
one thigh with opposite signs, the collision penalty counts it and termination does not, level 2 with no pair in reach is level 1 bit for bit,
a wavefront that holds touching and non-touching envs leaves the latter alone, calf-hip and calf-thigh rows work side by side, and a recorded
rollout equals the eager one.

Gaps are computed in float64 from DOF_STATE by tests/selfcol_thighs_ref.py, never from anything the kernel exports.  The drives were chosen on the
CPU with that reference on the oracle's trajectory (which has no such rows): no calf-calf, calf-hip or other calf-thigh pair comes within the
contact offset on the way.  QA_ENV_HELPERS is read once per process, so the scenarios run in two child processes (tests/test_selfcol_hips.py's
pattern); one child runs all of them and the tests share its result."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import selfcol_hips_ref as hips_ref
from tests import selfcol_thighs_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALF, THIGH, HIP = [5 + 4 * l for l in range(4)], [4 + 4 * l for l in range(4)], [3 + 4 * l for l in range(4)]
SLOP = -0.004            # the bound of the calf-calf and calf-hip tests: 4 sweeps, 5 ms substeps, the same depenetration cap
DEFAULT = np.array([0.0, 0.9, -1.8] * 4)
ACTION_SCALE = np.array([0.125, 0.25, 0.25] * 4)          # action_scale 0.25, halved on the hip joints


def _pose(**legs):
    q = DEFAULT.copy()
    for name, v in legs.items():
        l = ref.LEGS.index(name)
        q[3 * l:3 * l + 3] = v
    return q


def _action(target):
    return ((target - DEFAULT) / ACTION_SCALE).astype(np.float32)


# scenario -> (calf leg, thigh leg, start pose, PD target).  Targets are the isolated example poses of tests/selfcol_thighs_ref.py (a calf 40 mm
# inside the thigh, everything else of the pair 20 mm clear); the starts open the pair: on the oracle's trajectory the driven relation goes
# 34 mm / 43 mm deep while every other gap of the three classes stays above 41 mm / 20 mm.
SCENES = {
    "front_calf": (0, 2, _pose(FL=(-0.20, 1.73, -1.14), RL=(-0.50, 0.01, -1.01)), _pose(FL=(-0.50, 1.73, -1.14), RL=(-0.50, -0.39, -1.01))),
    "rear_calf": (2, 0, _pose(RL=(0.42, 0.01, -1.80), FL=(-0.47, 1.92, -1.15)), _pose(RL=(0.42, -0.49, -1.80), FL=(-0.47, 1.92, -1.15))),
}
# The momentum test's drive comes to REST (a knee opened to -1.15 rad leaves the explicit PD loop of the folded front leg in a
# velocity-clamped limit cycle, with or without any row -- the oracle shows it for both scenes above -- and the clamp is not momentum-neutral).
# Rear-left calf into the front-left thigh with the front knee at -1.52 rad: on the oracle's zero-gravity trajectory 31 mm deep, every other gap
# above 24 mm, every joint at rest (< 1e-3 rad/s) after 60 steps.
AT_REST = (2, 0, _pose(RL=(0.39, 0.08, -1.80), FL=(-0.39, 1.79, -1.52)), _pose(RL=(0.39, -0.42, -1.80), FL=(-0.39, 1.79, -1.52)))
# The front-left calf on the rear-left hip AND the rear-left thigh.  It starts inside the contact offset of both (thigh +1.4 mm, hip +6.8 mm) and
# opens its knee: on the oracle's trajectory 21 mm into the thigh and 33 mm into the hip, every other gap above 100 mm.  (Driven in from further
# away, whichever shape the calf meets first keeps it off the other.)  A hip force ends an episode, so this one runs through physics_step.
BOTH = (_pose(FL=(0.13, 2.05, -1.32), RL=(0.05, -0.18, -1.83)), _pose(FL=(0.13, 2.05, -1.02), RL=(0.05, -0.18, -1.83)))
# the joint-limit sweep's deepest calf-hip pose (profiles/self_collision_hips_sweep.json): the front calves 68 mm inside the rear hips
HIP_DEEP = _pose(FL=(0.0, 2.05, -0.87), FR=(0.0, 2.05, -0.87))

CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.oracle_lib import OracleSim, go2_cfg
from tests.test_self_collision import CROSS
from tests.test_selfcol_thighs import SCENES, AT_REST, BOTH, HIP_DEEP, DEFAULT, _action
from quadrupedal_agility_amd.sim import QaSim
out = sys.argv[1]
res = {}

def free_robots(n, poses, gravity=-9.81):
    # tests/test_self_collision.py::_free_robot for n envs: 40 m up, nothing resets, joints at `poses` (n, 12)
    q = go2_cfg(n, randomize_base_mass=0, randomize_base_com=0, randomize_motor=0, randomize_friction=0, gravity_z=gravity, push_robots=0, add_noise=0, self_collision=1)
    o = OracleSim(q); o.reset_all()
    o.t["ROOT_STATES"][:] = [0, 0, 40.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    o.t["DOF_STATE"][:, :, 0] = poses; o.t["DOF_STATE"][:, :, 1] = 0
    o.t["EPISODE_LENGTH"][:] = 5
    return q, o

def handle(q, o, level):
    h = QaSim(q, "cuda:0")
    h.arena.copy_(torch.from_numpy(o.arena.copy()).cuda()); h.global_step = o.global_step
    if level >= 1:
        h.set_self_collision_hips(True)
    if level >= 2:
        h.set_self_collision_thighs(True)
    return h

def finite(h):
    return all(bool(torch.isfinite(h.t[k]).all()) for k in ("ROOT_STATES", "DOF_STATE", "CONTACT_FORCES", "RIGID_BODY_POS"))

def drive(tag, start, target, level, steps=50, fused=True):
    # a constant action through the fused step (the kernels that have helper wavefronts; nothing may reset on the way) or the physics-only step
    q, o = free_robots(1, start[None]); h = handle(q, o, level)
    a = torch.from_numpy(_action(target)[None]).cuda()
    dof, cf, reset, ok = [], [], [], True
    for _ in range(steps):
        h.step(a) if fused else h.physics_step(a)
        torch.cuda.synchronize()
        dof.append(h.t["DOF_STATE"][0, :, 0].cpu().numpy()); cf.append(h.t["CONTACT_FORCES"][0].cpu().numpy()); reset.append(int(h.t["RESET"][0])); ok = ok and finite(h)
    res[f"{tag}{level}_dof"] = np.array(dof); res[f"{tag}{level}_cf"] = np.array(cf); res[f"{tag}{level}_reset"] = np.array(reset); res[f"{tag}{level}_finite"] = np.array(ok)

# cases 1, 2: a calf into the neighbour's thigh, both orderings; case 3: hip and thigh at once (level 0: neither row)
for tag, (a_, b_, start, target) in SCENES.items():
    for level in (1, 2):
        drive(tag, start, target, level)
for level in (0, 2):
    drive("both", BOTH[0], BOTH[1], level, steps=40, fused=False)

# case 4: zero gravity, no ground; the new class (level 2) and the calf-calf class (CROSS, level 0: the yardstick) by the same procedure
_, _, start, target = AT_REST
for tag, pose, act, level in (("mom_thighs", start, _action(target), 2), ("mom_calves", DEFAULT, CROSS, 0)):
    q, o = free_robots(1, pose[None], gravity=0.0)
    o.t["ROOT_STATES"][0, 7:13] = [0.3, -0.2, 0.1, 0.2, 0.1, -0.3]
    h = handle(q, o, level)
    a = torch.from_numpy(np.asarray(act, np.float32)[None]).cuda()
    for _ in range(10):
        h.physics_step(a)
    torch.cuda.synchronize()
    res[tag + "_root0"] = h.t["ROOT_STATES"][0].cpu().numpy(); res[tag + "_dof0"] = h.t["DOF_STATE"][0].cpu().numpy()
    cf, dof = [], []
    for _ in range(50):
        h.physics_step(a); torch.cuda.synchronize()
        cf.append(h.t["CONTACT_FORCES"][0].cpu().numpy()); dof.append(h.t["DOF_STATE"][0].cpu().numpy())
    res[tag + "_cf"] = np.array(cf); res[tag + "_dofs"] = np.array(dof)
    res[tag + "_root1"] = h.t["ROOT_STATES"][0].cpu().numpy(); res[tag + "_dof1"] = h.t["DOF_STATE"][0].cpu().numpy()

# case 5: the first fused step of an env that starts inside a thigh (env 0) next to one that starts inside a hip (env 1)
poses = np.stack([SCENES["rear_calf"][3], HIP_DEEP])
acts = np.stack([_action(SCENES["rear_calf"][3]), _action(HIP_DEEP)]).astype(np.float32)
for level in (1, 2):
    q, o = free_robots(2, poses); h = handle(q, o, level)
    h.step(torch.from_numpy(acts).cuda()); torch.cuda.synchronize()
    res[f"pen{level}_cf"] = h.t["CONTACT_FORCES"].cpu().numpy(); res[f"pen{level}_reset"] = h.t["RESET"].cpu().numpy()
    res[f"pen{level}_sums"] = h.t["EPISODE_SUMS"].cpu().numpy(); res[f"pen{level}_rew"] = h.t["REW"].cpu().numpy()
    res[f"pen{level}_scale"] = np.array(list(q.reward_scale_dt))

# case 6: 17 envs, one in thigh contact among 16 with random actions
n = 17
rng = np.random.default_rng(4)
acts = [(rng.normal(0, 0.5, (n, 12))).astype(np.float32) for _ in range(20)]
_, _, start, target = SCENES["front_calf"]
poses = np.tile(DEFAULT, (n, 1)); poses[0] = start
for a in acts:
    a[0] = _action(target)
for level in (1, 2):
    q, o = free_robots(n, poses); h = handle(q, o, level)
    dof = []
    for a in acts:
        h.step(torch.from_numpy(a).cuda()); torch.cuda.synchronize()
        dof.append(h.t["DOF_STATE"][:, :, 0].cpu().numpy())
    res[f"mixed{level}_dof"] = np.array(dof)
    for k, v in h.t.items():
        if v.dim() >= 1 and v.shape[0] == n:
            res[f"mixed{level}_T_{k}"] = v.cpu().numpy()
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the scenarios above, once per helper setting"""
    d = tmp_path_factory.mktemp("selfcol_thighs")
    outs = {}
    for mode in ("0", "1"):
        out = str(d / f"helpers{mode}.npz")
        subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], check=True, env=dict(os.environ, QA_ENV_HELPERS=mode), timeout=600)
        outs[mode] = np.load(out)
    return outs


def _other_classes(dof):
    """smallest calf-hip gap (all four front / rear relations) and calf-calf gap (all four neighbour pairs) of joint angles (..., 12)"""
    cc = [ref.calf_calf_gap(dof[..., 3 * a:3 * a + 3], a, dof[..., 3 * b:3 * b + 3], b) for a, b in [(0, 1), (2, 3), (0, 2), (1, 3)]]
    return float(hips_ref.all_gaps(dof).min()), float(np.min(cc))


@pytest.mark.parametrize("helpers", ["0", "1"])
@pytest.mark.parametrize("scene", ["front_calf", "rear_calf"])
def test_a_leg_driven_into_a_thigh_stops_at_the_surfaces(runs, helpers, scene):
    r = runs[helpers]
    a, b = SCENES[scene][:2]
    k = ref.ROW_RELATIONS.index((a, b))
    off, on = ref.all_gaps(r[scene + "1_dof"]), ref.all_gaps(r[scene + "2_dof"])
    print(scene, "calf-thigh gaps (m) of", ref.ROW_RELATIONS, "level 1 / level 2, min over 50 steps:", off.min(0), on.min(0))
    assert not r[scene + "1_reset"].any() and not r[scene + "2_reset"].any()
    assert bool(r[scene + "1_finite"]) and bool(r[scene + "2_finite"])
    # the drive is clean: at level 1 no calf-hip or calf-calf pair comes within the contact offset on the way, nor any other calf-thigh relation
    ch, cc = _other_classes(r[scene + "1_dof"])
    assert ch > ref.CONTACT_OFFSET and cc > ref.CONTACT_OFFSET and np.delete(off, k, axis=1).min() > ref.CONTACT_OFFSET, (ch, cc, off.min(0))
    assert off[:, k].min() < -0.010, off[:, k].min()            # without the rows the calf passes through the thigh
    assert on[:, k].min() > SLOP, on[:, k].min()                # with them it stops at the surfaces
    # the other side's pair is untouched: far apart, and no force on its thighs or calves
    side = [i for i, (x, _) in enumerate(ref.ROW_RELATIONS) if (x & 1) != (a & 1)]
    assert on[:, side].min() > ref.CONTACT_OFFSET
    cf = r[scene + "2_cf"]
    others = [CALF[l] for l in range(4) if (l & 1) != (a & 1)] + [THIGH[l] for l in range(4) if (l & 1) != (a & 1)]
    assert np.abs(cf[:, others]).max() == 0.0
    assert np.linalg.norm(cf[:, THIGH[b]], axis=-1).max() > 0.1 and np.abs(r[scene + "1_cf"][:, THIGH]).max() == 0.0


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
    """zero gravity, no ground, 10 settling steps, then 50: opposite forces on one calf and one thigh, nothing elsewhere, momentum unchanged.
    Procedure and bound of tests/test_selfcol_hips.py::test_the_contact_is_an_internal_force: the drift of the calf-calf class (CROSS, level 0)
    by the same procedure on the same kernels, times two.  profiles/self_collision_thighs_kats.json records both."""
    r = runs["0"]
    a, b = AT_REST[:2]
    cf = r["mom_thighs_cf"]
    for step in cf:
        assert np.allclose(step[CALF[a]], -step[THIGH[b]], atol=1e-4), (step[CALF[a]], step[THIGH[b]])
        assert np.abs(np.delete(step, [CALF[a], THIGH[b]], axis=0)).max() == 0.0
    peak = float(np.linalg.norm(cf[:, THIGH[b]], axis=-1).max())
    assert peak > 1.0, peak
    qd_end = float(np.abs(r["mom_thighs_dofs"][-5:, :, 1]).max())
    drift = {}
    for tag in ("mom_thighs", "mom_calves"):
        p0, L0 = _momentum(oracle_lib, r[tag + "_root0"], r[tag + "_dof0"]); p1, L1 = _momentum(oracle_lib, r[tag + "_root1"], r[tag + "_dof1"])
        drift[tag] = (float(np.abs(p1 - p0).max()), float(np.abs(L1 - L0).max()))
    assert float(np.abs(r["mom_calves_cf"][:, CALF]).max()) > 5.0          # the yardstick run did have its legs in contact
    print("momentum drift over 50 steps (linear kg m/s, angular kg m^2/s): calf-thigh", drift["mom_thighs"], "calf-calf", drift["mom_calves"],
          "peak thigh force (N)", peak, "largest joint speed over the last 5 steps (rad/s)", qd_end)
    assert drift["mom_thighs"][0] <= 2 * drift["mom_calves"][0] and drift["mom_thighs"][1] <= 2 * drift["mom_calves"][1], drift


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_the_penalty_sees_it_and_termination_does_not(runs, helpers):
    from quadrupedal_agility_amd._capi import REWARD_NAMES
    r = runs[helpers]
    a, b = SCENES["rear_calf"][:2]
    col = REWARD_NAMES.index("collision")
    assert r["pen2_scale"][col] != 0.0
    tf = np.linalg.norm(r["pen2_cf"][:, THIGH], axis=-1)           # (2 envs, 4 thighs)
    hf = np.linalg.norm(r["pen2_cf"][:, HIP], axis=-1)
    print("first step: thigh forces (N)", tf, "hip forces (N)", hf, "RESET", r["pen2_reset"], "collision sums", r["pen2_sums"][col], "REW", r["pen2_rew"])
    assert tf[0, b] > 0.1 and hf[0].max() == 0.0
    assert r["pen2_sums"][col, 0] != 0.0 and r["pen2_reset"][0] == 0          # penalised, not terminated
    assert hf[1].max() > 1.0 and r["pen2_reset"][1] == 1                       # the hip row of the neighbouring env still ends its episode
    # level 1 on the same launch: no thigh force, no penalty, the same termination
    assert np.abs(r["pen1_cf"][0, THIGH]).max() == 0.0 and r["pen1_sums"][col, 0] == 0.0
    assert list(r["pen1_reset"]) == [0, 1] and np.linalg.norm(r["pen1_cf"][1, HIP], axis=-1).max() > 1.0


@pytest.mark.parametrize("helpers", ["0", "1"])
def test_mixed_wavefront_leaves_the_other_envs_alone(runs, helpers):
    r = runs[helpers]
    n = 17
    driven = np.arange(n) == 0
    names = [k[len("mixed1_T_"):] for k in r.files if k.startswith("mixed1_T_")]
    assert "DOF_STATE" in names and "ROOT_STATES" in names and "CONTACT_FORCES" in names
    for k in names:
        x, y = r["mixed1_T_" + k], r["mixed2_T_" + k]
        assert np.array_equal(x[~driven], y[~driven], equal_nan=True), k        # the wave-uniform vote does not leak into lanes whose pair is apart
    assert np.array_equal(r["mixed1_dof"][:, ~driven], r["mixed2_dof"][:, ~driven])
    on, off = ref.all_gaps(r["mixed2_dof"][:, driven]), ref.all_gaps(r["mixed1_dof"][:, driven])
    assert off[..., 0].min() < -0.010 and on[..., 0].min() > SLOP, (off[..., 0].min(), on[..., 0].min())
    assert ref.all_gaps(r["mixed2_dof"][:, ~driven]).min() > ref.CONTACT_OFFSET     # (and the random-action envs were indeed apart)


def test_hip_and_thigh_rows_side_by_side(runs):
    """the front-left calf lies on the rear-left hip AND the rear-left thigh (physics-only step: helper wavefronts play no part)"""
    r = runs["0"]
    th0, th2 = ref.all_gaps(r["both0_dof"])[:, 0], ref.all_gaps(r["both2_dof"])[:, 0]
    hp0, hp2 = hips_ref.all_gaps(r["both0_dof"])[:, 0], hips_ref.all_gaps(r["both2_dof"])[:, 0]
    print("FL calf on RL thigh / RL hip, min gap (m): no rows", th0.min(), hp0.min(), "level 2", th2.min(), hp2.min())
    assert th0.min() < -0.010 and hp0.min() < -0.010             # without the rows the pose does reach both
    assert bool(r["both2_finite"]) and np.isfinite(r["both2_dof"]).all()
    assert th2.min() > SLOP and hp2.min() > SLOP
    cf = r["both2_cf"]
    assert np.linalg.norm(cf[:, THIGH[2]], axis=-1).max() > 0.1 and np.linalg.norm(cf[:, HIP[2]], axis=-1).max() > 0.1      # both rows did carry force


def _random_steps(h, n, steps, seed, record=None):
    import torch
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        h.step((torch.randn(n, 12, generator=g) * 0.5).cuda())
        if record is not None:
            record.append(h.t["DOF_STATE"][:, :, 0].cpu().numpy())
    torch.cuda.synchronize()


def _set_level(h, level):
    if level >= 1:
        h.set_self_collision_hips(True)
    if level >= 2:
        h.set_self_collision_thighs(True)


def test_off_is_off_on_the_plane():
    """17 envs: the last (only) wavefront is partial.  40 random-action steps from reset_all(): level 2 = level 1 = level 0 bit for bit on the
    whole arena, and no calf-thigh pair comes within the contact offset"""
    import torch
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import go2_cfg
    n = 17
    arenas, dofs = [], []
    for level in (2, 1, 0):
        h = QaSim(go2_cfg(n, seed=3, self_collision=1), "cuda:0")
        _set_level(h, level)
        h.reset_all()
        rec = []
        _random_steps(h, n, 40, seed=8, record=rec)
        arenas.append(h.arena.clone()); dofs.append(np.array(rec))
    assert ref.all_gaps(dofs[0]).min() > ref.CONTACT_OFFSET, ref.all_gaps(dofs[0]).min()
    assert torch.equal(arenas[0], arenas[1])
    assert torch.equal(arenas[1], arenas[2])


def test_off_is_off_on_a_height_field_and_through_simulate():
    """the same on a height-field handle (tests/test_hip_parity.py::make_terrain_pair's config), with one qa_simulate at the end"""
    import torch
    from tests.test_hip_parity import make_terrain_pair, push_arena
    n = 17
    arenas = []
    for level in (2, 1):
        q, o, h = make_terrain_pair(n, 5, self_collision=1)
        o.reset_all()
        push_arena(o, h)
        _set_level(h, level)
        rec = []
        _random_steps(h, n, 40, seed=9, record=rec)
        h.simulate(torch.zeros(n, 12, device="cuda")); torch.cuda.synchronize()
        arenas.append(h.arena.clone())
        assert ref.all_gaps(np.array(rec)).min() > ref.CONTACT_OFFSET
    assert torch.equal(arenas[0], arenas[1])


def test_setter_contract():
    """NULL handle, a handle without self_collision, and the level's transitions seen through what one physics step reports: from a pose inside a
    hip and a thigh, level 2 reports both forces, level 1 the hip's only, level 0 neither"""
    import torch
    from quadrupedal_agility_amd import _capi
    from quadrupedal_agility_amd.sim import QaSim
    from tests.oracle_lib import OracleSim, go2_cfg
    lib = _capi.load_library()
    assert lib.qa_set_self_collision_thighs(None, 1) == -1 and lib.qa_set_self_collision_thighs(None, 0) == -1
    h = QaSim(go2_cfg(4, self_collision=0), "cuda:0")
    with pytest.raises(RuntimeError, match="self_collision"):
        h.set_self_collision_thighs(True)                  # QA_E_ARG: the handle has no self-collision model
    h.set_self_collision_thighs(False)
    q = go2_cfg(1, randomize_base_mass=0, randomize_base_com=0, randomize_motor=0, randomize_friction=0, push_robots=0, add_noise=0, self_collision=1)
    o = OracleSim(q); o.reset_all()
    o.t["ROOT_STATES"][:] = [0, 0, 40.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    o.t["DOF_STATE"][:, :, 0] = BOTH[1]; o.t["DOF_STATE"][:, :, 1] = 0
    h = QaSim(q, "cuda:0")
    start = torch.from_numpy(o.arena.copy()).cuda()
    act = torch.from_numpy(_action(BOTH[1])[None]).cuda()

    def probe():
        h.arena.copy_(start)
        h.physics_step(act); torch.cuda.synchronize()
        cf = h.t["CONTACT_FORCES"][0].cpu().numpy()
        return bool(np.abs(cf[HIP]).max() > 0), bool(np.abs(cf[THIGH]).max() > 0)
    assert probe() == (False, False)
    h.set_self_collision_thighs(False); assert probe() == (False, False)         # 0 stays 0
    h.set_self_collision_thighs(True); assert probe() == (True, True) and h.self_collision_hips and h.self_collision_thighs       # 0 -> 2
    h.set_self_collision_thighs(False); assert probe() == (True, False) and h.self_collision_hips and not h.self_collision_thighs  # 2 -> 1
    h.set_self_collision_thighs(False); assert probe() == (True, False)          # 1 stays 1
    h.set_self_collision_hips(False); assert probe() == (False, False)           # 1 -> 0
    h.set_self_collision_thighs(True); h.set_self_collision_hips(True); assert probe() == (True, False)      # the hips' setter sets 1, as it always did
    h.set_self_collision_thighs(True); h.set_self_collision_hips(False); assert probe() == (False, False) and not h.self_collision_thighs


def test_recorded_rollout_equals_eager_rollout(monkeypatch):
    """small BBC rollouts at level 2: hipGraph replays of the rollout against eager launches, the env arena bit for bit (the pattern of
    tests/test_selfcol_hips.py::test_recorded_rollout_equals_eager_rollout)"""
    import torch
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    res = []
    for graph in ("1", "0"):
        monkeypatch.setenv("QA_ROLLOUT_GRAPH", graph)
        np.random.seed(0); torch.manual_seed(0)
        cfg = Go2LocomotionCfg(); cfg.env.num_envs = 64; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
        cfg.asset.qa_self_collision_hips = True; cfg.asset.qa_self_collision_thighs = True
        t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = False
        args = get_args(["--device", "gpu"])
        env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
        assert env.self_collision_thighs and env.sim.self_collision_thighs and env.sim.self_collision_hips
        runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=None)
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        assert (runner._graph is not None and not runner._graph_failed) == (graph == "1")
        res.append(env.sim.arena.clone())
    assert torch.equal(res[0], res[1])          # the env's whole state after two rollouts: observations, rewards, resets, contact forces
