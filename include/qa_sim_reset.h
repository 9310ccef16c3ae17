/* qa_sim_reset.h -- extension of include/qa_sim.h: recovery-pose resets (env.recovery_init_prob) inside the fused env step, and the body
 * classes that end an episode / count for the collision penalty (asset.terminate_after_contacts_on, asset.penalize_contacts_on).
 *
 * Kept apart from qa_sim.h for the reason qa_sim_rewards.h is: that header is the ABI the CPU oracle twins symbol by symbol
 * (tests/test_abi.py), and this feature adds neither an arena tensor nor a config field to it.  The library exports the entry points next to
 * the ABI; the Python side binds them through _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_SIM_RESET_H
#define QA_SIM_RESET_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Recovery-pose resets (bbc/legged_gym/envs/base/legged_robot.py:205-214, 636-658).  With prob > 0 every kernel that resets envs -- the
 * fused step (qa_env_step / qa_env_step_dev, plane and height field, with and without the terrain curriculum), qa_debug_post_physics and
 * qa_reset_all -- takes ONE decision per global step, the same for every env of the launch and for every rank of a job:
 *     recovery = U < prob,   U = the first value of the handle's Philox stream 14 at (env word 0xFFFFFFFF, step, block 0).
 * The env word is no global env id, so cfg.env_id_offset does not enter: every env and every rank draws the same number, as the reference
 * draws one np.random.random() per reset_idx call.  The reference compares with <=; < keeps "0 = never, 1 = always" exact (U lies in
 * [0, 1)), and the two differ on a set of measure zero.  With prob == 0 the draw is not made.
 *
 * On a step whose decision is yes, every env that resets is thrown in tumbled instead of taking the handle's reset_mode path.  33 uniforms
 * of stream 14 at (global env id, step, blocks 1..9), in the reference's call order, fp32 as torch_rand_float writes it ((hi - lo) * u + lo):
 *     u[0:12]   dof_pos  = default_dof_pos * (1.5 u + 0.5)      joint 3 * leg + k; NOT clamped to the joint limits (the stop rows act)
 *     u[12:24]  dof_vel  = 2 u - 1
 *     u[24:30]  root linear, then angular velocity = u - 0.5, world frame
 *     u[30:33]  roll, pitch, yaw = 6.28 u - 3.14; the quaternion by quat_from_euler_xyz (torch_jit_utils.py:46), not renormalised
 *     position  = init_pos + the env's origin (where the terrain curriculum has just moved it: the new origin); no xy jitter
 * Commands, latents, episode sums, air time and histories are handled as any reset handles them.  On a step whose decision is no, the
 * handle's reset_mode path runs unchanged, bit for bit.
 *
 * The probability travels in the launch arguments.  A recorded rollout (hipGraph) bakes it in: call this BEFORE the first recording, and
 * record again after changing it.  Works on handles of either reset_mode, on plane and on height-field handles.
 * Returns QA_E_ARG on a NULL handle and on prob outside [0, 1] (NaN included). */
int qa_set_recovery_init(qa_sim *sim, float prob);

/* Body classes of the Go2 whose contact forces the post-physics phase holds.  The Head bodies carry no contact points in this model. */
#define QA_BC_BASE  1u
#define QA_BC_HIP   2u
#define QA_BC_THIGH 4u
#define QA_BC_CALF  8u
#define QA_BC_FOOT  16u
#define QA_BC_ALL   31u
#define QA_BC_DEFAULT_TERMINATION (QA_BC_BASE | QA_BC_HIP)
#define QA_BC_DEFAULT_PENALISED   (QA_BC_THIGH | QA_BC_CALF)

/* check_termination (legged_robot.py:168-176) ends the episode when a body of a class in termination_mask carries |f| > 1 N;
 * _reward_collision (:1267) counts the bodies of the classes in penalised_mask with |f| > 0.1 N: the base once per env, a leg class once
 * per leg.  The defaults are what the kernels did before this call existed (QA_BC_DEFAULT_*), and with them every arena tensor is
 * bit-identical to never having called it.  The fused step and qa_debug_post_physics read the masks; time-outs and the non-finite guard
 * are not affected.
 *
 * The masks travel in the launch arguments: call this BEFORE the first recording, and record again after a change.
 * Returns QA_E_ARG on a NULL handle and on bits outside QA_BC_ALL. */
int qa_set_contact_sets(qa_sim *sim, uint32_t termination_mask, uint32_t penalised_mask);

#ifdef __cplusplus
}
#endif
#endif
