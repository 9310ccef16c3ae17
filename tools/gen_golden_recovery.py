#!/usr/bin/env python3
"""tests/golden/recovery_init.npz: what include/qa_sim_reset.h twins, as THE REFERENCE'S OWN PYTHON computes it.

Build container only (needs the reference checkout, like tools/gen_golden.py whose stub env and tools/ref_shims this reuses).  Data only.
  1. The reference's _reset_dofs_rec and _reset_root_states_rec (legged_robot.py:636-658) on all 64 envs with non-zero env origins.  The
     module's torch_rand_float is wrapped to record the uniforms it drew (the arithmetic stays the reference's (hi - lo) * u + lo); written:
     the 33 uniforms per env in call order, the origins, and the resulting root_states, dof_pos, dof_vel.
  2. The reference's post_physics_step on the mid-step arena of tests/golden/extra_rewards.npz with forces placed on a base, a hip, a thigh,
     a calf and a foot in different envs, under six pairs of asset.terminate_after_contacts_on / penalize_contacts_on (the index tensors
     built by the substring rule of legged_robot.py:1034-1039): reset_buf, time_out_buf, rew_buf and _reward_collision's return per pair.
     The forces are written as (env, body row, force) edits on top of that fixture's CONTACT_FORCES.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden as gg                      # noqa: E402

N = 64
PAIRS = [(["base", "hip"], ["thigh", "calf"]),             # the Go2 defaults
         ([], []),
         (["hip"], ["base", "thigh", "calf"]),
         (["calf", "foot"], ["hip"]),
         (["base"], ["foot", "thigh"]),
         (["base", "hip", "thigh", "calf", "foot"], ["base", "hip", "thigh", "calf", "foot"])]
# (env, body row of CONTACT_FORCES, force): one class per env, above 1 N, between 0.1 and 1 N, and below 0.1 N
EDITS = [(2, 0, [0.0, 0.0, 40.0]), (3, 0, [0.3, 0.0, 0.4]), (4, 0, [0.05, 0.0, 0.05]),          # base
         (20, 7, [1.5, 0.0, 0.5]), (21, 15, [0.0, 0.2, 0.0]),                                    # FR hip, RR hip
         (22, 4, [0.0, 3.0, 1.0]), (23, 12, [0.0, 0.5, 0.0]), (24, 8, [0.01, 0.0, 0.0]),         # FL thigh, RL thigh, FR thigh
         (25, 17, [2.0, 2.0, 2.0]), (26, 5, [0.0, 0.0, 0.15]),                                   # RR calf, FL calf
         (27, 6, [0.0, 0.0, 0.5]), (28, 18, [0.0, 0.0, 0.05]),                                   # FL foot below 1 N, RR foot below 0.1 N
         (29, 0, [0.0, 0.0, 5.0]), (29, 9, [0.0, 0.0, 5.0]), (29, 10, [0.0, 0.0, 90.0])]         # several classes in one env
QUIET = [2, 3, 4] + list(range(20, 30))      # these envs carry nothing but the edits (and their feet)


def golden_arena():
    g = np.load(os.path.join(ROOT, "tests", "golden", "extra_rewards.npz"), allow_pickle=False)
    a = {k[3:]: g[k].copy() for k in g.files if k.startswith("in_")}
    cf = a["CONTACT_FORCES"]
    cf[QUIET, :6] = 0.0; cf[QUIET, 7:10] = 0.0; cf[QUIET, 11:14] = 0.0; cf[QUIET, 15:18] = 0.0      # every non-foot body
    for env, body, f in EDITS:
        cf[env, body] = f
    return a


def part_reset(ref_lr, RefCfg, arena, out):
    env = gg.make_ref_env(ref_lr, RefCfg, N, arena)
    rng = np.random.default_rng(14)
    env.env_origins = torch.tensor(rng.uniform(-6.0, 6.0, (N, 3)).astype(np.float32))
    drawn = []
    plain = ref_lr.torch_rand_float

    def recording(lower, upper, shape, device):
        u = torch.rand(*shape, device=device)
        drawn.append(u.clone())
        return (upper - lower) * u + lower
    # the wrapper restates the shim's one line so that u is visible; checked against the shim itself below
    torch.manual_seed(3); a = plain(-3.14, 3.14, (5, 3), "cpu")
    torch.manual_seed(3); b = recording(-3.14, 3.14, (5, 3), "cpu")
    assert torch.equal(a, b)
    drawn.clear()
    ref_lr.torch_rand_float = recording
    if not hasattr(ref_lr.gymtorch, "unwrap_tensor"):          # the two functions hand their tensors to the (stubbed) simulator
        ref_lr.gymtorch.unwrap_tensor = lambda t: t
    try:
        torch.manual_seed(14)
        ids = torch.arange(N)
        env._reset_dofs_rec(ids)
        env._reset_root_states_rec(ids)
    finally:
        ref_lr.torch_rand_float = plain
    assert [tuple(d.shape) for d in drawn] == [(N, 12), (N, 12), (N, 6), (N, 3)]
    out.update(reset_uniforms=torch.cat(drawn, dim=1).numpy(), reset_env_origins=env.env_origins.numpy(),
               reset_root_states=env.root_states.numpy().copy(), reset_dof_pos=env.dof_pos.numpy().copy(), reset_dof_vel=env.dof_vel.numpy().copy(),
               reset_default_dof_pos=env.default_dof_pos.numpy()[0], reset_init_pos=np.array(env.cfg.init_state.pos, np.float32))
    q = env.root_states[:, 3:7].norm(dim=1)
    print("part 1: 64 envs, |quat| in", float(q.min()), float(q.max()), "calf range", float(env.dof_pos[:, 2::3].min()), float(env.dof_pos[:, 2::3].max()))


def part_contact_sets(ref_lr, RefCfg, arena, out):
    names = gg.BODY_NAMES
    noop = lambda self, *a, **k: None
    for i, (term, pen) in enumerate(PAIRS):
        env = gg.make_ref_env(ref_lr, RefCfg, N, arena)
        sel = lambda lst: torch.tensor([names.index(s) for name in lst for s in names if name in s], dtype=torch.long)
        env.termination_contact_indices, env.penalised_contact_indices = sel(term), sel(pen)
        for m in ("_resample_commands", "_resample_latent_eps", "_resample_latent_c", "_reset_dofs", "_reset_root_states", "_push_robots"):
            setattr(env, m, types.MethodType(noop, env))
        assert set(env.reward_names) <= set(gg_reward_names()), env.reward_names
        col = env._reward_collision().numpy().copy()
        env.post_physics_step()
        out[f"pair{i}_reset"] = env.reset_buf.numpy().astype(bool)
        out[f"pair{i}_time_out"] = env.time_out_buf.numpy().astype(bool)
        out[f"pair{i}_rew"] = env.rew_buf.numpy().copy()
        out[f"pair{i}_collision"] = col.astype(np.int64)
        assert (col == col.astype(np.int64)).all()
        out[f"pair{i}_terminate_on"] = np.array(term, dtype="U8")
        out[f"pair{i}_penalize_on"] = np.array(pen, dtype="U8")
        print(f"pair {i}: {term} / {pen}: resets {np.nonzero(out[f'pair{i}_reset'])[0].tolist()}, collision counts {sorted(set(col.tolist()))}")
    out["num_pairs"] = np.array(len(PAIRS))


def gg_reward_names():
    from quadrupedal_agility_amd import _capi
    return _capi.REWARD_NAMES


def main():
    ref_lr, RefCfg, _ = gg.import_reference()
    arena = golden_arena()
    out = {"edit_env": np.array([e for e, _, _ in EDITS]), "edit_body": np.array([b for _, b, _ in EDITS]),
           "edit_force": np.array([f for _, _, f in EDITS], np.float32), "quiet_envs": np.array(QUIET)}
    part_reset(ref_lr, RefCfg, arena, out)
    part_contact_sets(ref_lr, RefCfg, arena, out)
    resets = np.stack([out[f"pair{i}_reset"] for i in range(len(PAIRS))])
    assert (resets != resets[0]).any(axis=1).sum() >= 4, "the pairs must end different envs"
    path = os.path.join(ROOT, "tests", "golden", "recovery_init.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
