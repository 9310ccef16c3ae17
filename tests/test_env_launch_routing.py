"""-m gpu: every launch of the env engine reaches the instantiation it names.  The host side picks a kernel by self-collision level (the launcher
table k_levels of csrc/qa_sim.hip, one translation unit per level), terrain, lean mask, helper wavefronts and extra rewards; this test runs the
whole grid and recognises each axis by its documented signature, never by a stored number:

  lean            sentinels in TORQUES survive exactly when the mask is non-zero, sentinels in OBS_DISC exactly when it is 3
  extra rewards   the extra-reward sums buffer changes exactly when they are on
  both            leave ROOT_STATES, DOF_STATE, OBS, REW and RESET as lean 0 / extra rewards off has them, bit for bit
  level           DOF_STATE of the envs driven into a hip differs between levels 0 and 1, of those driven into a thigh between 1 and 2
  terrain         root heights differ between the plane and the height field
  physics_step, simulate, simulate_if: once per level and terrain, each level differs from the one below on the driven envs

Every fourth env gets the calf-into-hip drive of tests/test_selfcol_hips.py, every fourth-plus-one the calf-into-thigh drive of
tests/test_selfcol_thighs.py (both 40 m up, where nothing else touches them), the others stand on the ground with small random actions; 20 steps,
what those tests' mixed-wavefront cases take to reach contact.  64 envs fill their workgroups, 67 leave one partly filled.

The extra reward terms run with scales of 1e-30.  A term times such a scale is a normal fp32 number, so the sums buffer moves off zero; added
to a partial reward of 1e-22 or more it is below half an ulp, so REW keeps its bits -- which is what lets the test hold REW to the run without
the terms.  Two terms have no scale: termination, the one term that is added AFTER the only-positive clip, to what may be an exact zero; and
feet_air_time, which has a side effect by design, as in the reference -- with a scale it replaces LAST_CONTACTS' force-norm test by
force z > 1 N (csrc/qa_sim.hip, `contact_out = contact_z`), and the contact flags of OBS follow it.

QA_ENV_HELPERS is read once per process: one child per value, each under its own timeout (tests/test_env_helpers.py's pattern); one child runs
the whole grid and the tests share its result."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVELS, TERRAINS, LEANS, XRS, SIZES = (0, 1, 2), (0, 1), (0, 1, 3), (0, 1), (64, 67)
STEPS = 20
STATE = ("ROOT_STATES", "DOF_STATE", "OBS", "REW", "RESET")
SENTINEL = 12345.0           # no torque (effort limits are tens of N m) and no discriminator observation comes near it
XR_SCALE = 1e-30


def key(level, hf, lean, xr, n):
    return f"L{level}_T{hf}_M{lean}_X{xr}_N{n}_"


CHILD = r"""
import hashlib, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from quadrupedal_agility_amd import _capi
from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import ExtraRewards
from quadrupedal_agility_amd.sim import QaSim
from tests.oracle_lib import OracleSim, go2_cfg
from tests.test_hip_parity import make_terrain_pair
from tests.test_selfcol_hips import DRIVE
from tests.test_selfcol_thighs import SCENES, DEFAULT, _action
from tests.test_env_launch_routing import LEVELS, TERRAINS, LEANS, XRS, SIZES, STEPS, STATE, SENTINEL, XR_SCALE, key
out = sys.argv[1]
res = {}
OVER = dict(randomize_base_mass=0, randomize_base_com=0, randomize_motor=0, randomize_friction=0, push_robots=0, add_noise=0, self_collision=1)
_, _, T_START, T_TARGET = SCENES["front_calf"]

def start(n, hf):
    # the oracle's reset on the plane / on a rough field (tests/test_hip_parity.py), then the driven envs lifted out of everything's reach
    if hf:
        q, o, _ = make_terrain_pair(n, 5, with_hip=False, **OVER)
    else:
        q = go2_cfg(n, seed=5, **OVER); o = OracleSim(q)
    o.reset_all()
    hip, thigh = np.arange(n) %% 4 == 0, np.arange(n) %% 4 == 1
    o.t["ROOT_STATES"][hip | thigh, 2:] = [40.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    o.t["DOF_STATE"][hip, :, 0] = DEFAULT; o.t["DOF_STATE"][thigh, :, 0] = T_START; o.t["DOF_STATE"][hip | thigh, :, 1] = 0
    o.t["EPISODE_LENGTH"][:] = 5
    rng = np.random.default_rng(4)
    acts = [rng.normal(0, 0.5, (n, 12)).astype(np.float32) for _ in range(STEPS)]
    for a in acts:
        a[hip] = DRIVE; a[thigh] = _action(T_TARGET)
    return q, torch.from_numpy(o.arena.copy()).cuda(), o.global_step, [torch.from_numpy(a).cuda() for a in acts]

def handle(q, arena, step, level):
    h = QaSim(q, "cuda:0")
    h.arena.copy_(arena); h.global_step = step
    if level >= 1:
        h.set_self_collision_hips(True)
    if level >= 2:
        h.set_self_collision_thighs(True)
    return h

def sha(t):
    return np.array(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest())

scales = [XR_SCALE] * _capi.NUM_EXTRA_REWARDS
for name in ("termination", "feet_air_time"):
    scales[_capi.EXTRA_REWARD_NAMES.index(name)] = 0.0
for n in SIZES:
    for hf in TERRAINS:
        q, arena, step0, acts = start(n, hf)
        for level in LEVELS:
            for lean in LEANS:
                for xr in XRS:
                    h = handle(q, arena, step0, level)
                    h.set_extra_rewards(ExtraRewards(scales, 0.3, 100.0, 0.02, None))
                    sums = h.extra_episode_sums            # the buffer outlives the switch-off below
                    if not xr:
                        h.set_extra_rewards(None)
                    h.set_lean_exports(lean)
                    h.t["TORQUES"].fill_(SENTINEL); h.t["OBS_DISC"].fill_(SENTINEL)
                    before = sums.clone()
                    for a in acts:
                        h.step(a)
                    torch.cuda.synchronize()
                    k = key(level, hf, lean, xr, n)
                    for name in STATE:
                        res[k + name] = h.t[name].cpu().numpy()
                    for name in ("TORQUES", "OBS_DISC"):
                        s = h.t[name] == SENTINEL
                        res[k + name + "_kept"] = np.array([bool(s.all()), bool(s.any())])
                    res[k + "xr_changed"] = np.array(not torch.equal(sums, before))
                    res[k + "xr_sums"] = sums.cpu().numpy()
                    for name, v in h.t.items():            # every tensor of the arena, for comparisons of two builds of the library
                        res[k + "sha_" + name] = sha(v)
        if n != SIZES[-1]:
            continue
        # the physics-only step and qa_simulate / qa_simulate_if, once per level and terrain.  The simulate calls of EVERY level start from the
        # arena level 0's physics steps end in: the driven calves inside the hip / the thigh
        deep = None
        for level in LEVELS:
            h = handle(q, arena, step0, level)
            for a in acts:
                h.physics_step(a)
            torch.cuda.synchronize()
            k = f"L{level}_T{hf}_"
            res[k + "phys_dof"] = h.t["DOF_STATE"].cpu().numpy(); res[k + "phys_sha"] = sha(h.arena)
            if level == 0:
                deep = h.arena.clone()
            h.arena.copy_(deep)
            tau = h.t["TORQUES"].clone()
            for _ in range(4):
                h.simulate(tau)
            torch.cuda.synchronize()
            res[k + "sim_dof"] = h.t["DOF_STATE"].cpu().numpy(); res[k + "sim_sha"] = sha(h.arena)
            h.arena.copy_(deep)
            for _ in range(4):
                h.simulate_if(tau, torch.ones(1, dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            res[k + "simif_dof"] = h.t["DOF_STATE"].cpu().numpy(); res[k + "simif_sha"] = sha(h.arena)
            h.arena.copy_(deep)
            h.simulate_if(tau, torch.zeros(1, dtype=torch.uint8, device="cuda")); torch.cuda.synchronize()
            res[k + "simif0_same"] = np.array(torch.equal(h.arena, deep))
np.savez(out, **res)
"""


def run_children(directory, env=None):
    """the grid, once per helper setting -> {"0": npz, "1": npz}"""
    outs = {}
    for mode in ("0", "1"):
        out = os.path.join(str(directory), f"helpers{mode}.npz")
        subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], check=True, env=dict(env or os.environ, QA_ENV_HELPERS=mode), timeout=600)
        outs[mode] = np.load(out)
    return outs


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return run_children(tmp_path_factory.mktemp("env_launch_routing"))


GRID = list(itertools.product(LEVELS, TERRAINS, LEANS, XRS, SIZES))
HELPERS = pytest.mark.parametrize("helpers", ["0", "1"])


@HELPERS
def test_lean_masks_skip_exactly_their_exports(runs, helpers):
    r = runs[helpers]
    for level, hf, lean, xr, n in GRID:
        k = key(level, hf, lean, xr, n)
        t_all, t_any = r[k + "TORQUES_kept"]
        d_all, d_any = r[k + "OBS_DISC_kept"]
        assert (t_all, t_any) == ((True, True) if lean else (False, False)), (k, t_all, t_any)         # kept whole, or written whole
        assert (d_all, d_any) == ((True, True) if lean == 3 else (False, False)), (k, d_all, d_any)


@HELPERS
def test_extra_reward_sums_move_exactly_when_the_terms_are_on(runs, helpers):
    r = runs[helpers]
    for level, hf, lean, xr, n in GRID:
        k = key(level, hf, lean, xr, n)
        assert bool(r[k + "xr_changed"]) == bool(xr), k


@HELPERS
def test_lean_and_extra_rewards_leave_the_state_alone(runs, helpers):
    r = runs[helpers]
    for level, hf, lean, xr, n in GRID:
        base, k = key(level, hf, 0, 0, n), key(level, hf, lean, xr, n)
        for name in STATE:
            assert np.array_equal(r[base + name], r[k + name], equal_nan=True), (k, name)
        assert np.isfinite(r[k + "ROOT_STATES"]).all() and np.isfinite(r[k + "DOF_STATE"]).all(), k


def _levels_differ(get, n, what):
    """each level against the one below, on the envs whose drive that level's rows stop; a pair of levels that agrees everywhere means the drive
    never reached contact (or the launch never reached the level's kernels)"""
    hip, thigh = np.arange(n) % 4 == 0, np.arange(n) % 4 == 1
    l0, l1, l2 = (get(level) for level in LEVELS)
    assert l0.shape == (n, 12, 2)
    moved = (l0[hip] != l1[hip]).any(axis=(1, 2))
    assert moved.all(), (what, "levels 0 and 1 agree on hip-driven envs", np.flatnonzero(hip)[~moved])
    moved = (l1[thigh] != l2[thigh]).any(axis=(1, 2))
    assert moved.all(), (what, "levels 1 and 2 agree on thigh-driven envs", np.flatnonzero(thigh)[~moved])
    assert np.array_equal(l0[thigh], l1[thigh]), (what, "the calf-hip rows moved a thigh-driven env")     # level 1 has no row for that pair


@HELPERS
def test_each_level_reaches_its_own_kernels(runs, helpers):
    r = runs[helpers]
    for hf, lean, xr, n in itertools.product(TERRAINS, LEANS, XRS, SIZES):
        _levels_differ(lambda level: r[key(level, hf, lean, xr, n) + "DOF_STATE"], n, key("*", hf, lean, xr, n))


@HELPERS
def test_plane_and_height_field_kernels_differ(runs, helpers):
    r = runs[helpers]
    for level, lean, xr, n in itertools.product(LEVELS, LEANS, XRS, SIZES):
        plane, field = (r[key(level, hf, lean, xr, n) + "ROOT_STATES"][:, 2] for hf in TERRAINS)
        ground = np.arange(n) % 4 >= 2                       # the envs that stand on the terrain
        assert (plane[ground] != field[ground]).all(), key(level, "*", lean, xr, n)


@HELPERS
def test_physics_step_and_simulate_reach_each_level(runs, helpers):
    r = runs[helpers]
    n = SIZES[-1]
    for hf in TERRAINS:
        for what in ("phys", "sim", "simif"):
            _levels_differ(lambda level: r[f"L{level}_T{hf}_{what}_dof"], n, f"{what} T{hf}")
        for level in LEVELS:
            assert bool(r[f"L{level}_T{hf}_simif0_same"])                                          # qa_simulate_if with a zero condition is a no-op
            assert np.array_equal(r[f"L{level}_T{hf}_sim_dof"], r[f"L{level}_T{hf}_simif_dof"])    # and with a non-zero one it is qa_simulate
