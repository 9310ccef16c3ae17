/* qa_tsc_rewards.h -- extension of include/qa_sim.h: the task-level tree's other fourteen reward terms inside the goal step.
 *
 * A sibling of qa_sim_rewards.h (the behaviour-level tree's ten) and kept apart from qa_sim.h for the same reason: that header is the
 * ABI the CPU oracle twins symbol by symbol (tests/test_abi.py), and this feature changes neither qa_tsc_goal_cfg nor qa_tsc_goal_io
 * nor QA_TSC_NUM_REWARDS.  The library exports the entry point next to the ABI; the Python side binds it through
 * _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_TSC_REWARDS_H
#define QA_TSC_REWARDS_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The terms, in alphabetical order (tsc/legged_gym/envs/base/legged_robot.py, the line of each _reward_* function):
 *   action_rate :1844, ang_vel_xy :1829, delta_torques :1861, dof_acc :1837, dof_error :1889, dof_pos_limits :1872,
 *   dof_vel_limits :1878, every_step :1924, feet_stumble :1893, hip_pos :1885, lin_vel_z :1824, orientation :1832,
 *   torque_limits :1867, torques :1864.
 * With the eight of qa_tsc_goal_step (QA_TSC_REW_*) these are the reference's 22. */
#define QA_TSC_NUM_EXTRA_REWARDS 14
enum {
    QA_TSC_XR_ACTION_RATE = 0, QA_TSC_XR_ANG_VEL_XY, QA_TSC_XR_DELTA_TORQUES, QA_TSC_XR_DOF_ACC, QA_TSC_XR_DOF_ERROR, QA_TSC_XR_DOF_POS_LIMITS,
    QA_TSC_XR_DOF_VEL_LIMITS, QA_TSC_XR_EVERY_STEP, QA_TSC_XR_FEET_STUMBLE, QA_TSC_XR_HIP_POS, QA_TSC_XR_LIN_VEL_Z, QA_TSC_XR_ORIENTATION,
    QA_TSC_XR_TORQUE_LIMITS, QA_TSC_XR_TORQUES
};

typedef struct qa_tsc_extra_rewards {
    float scale_dt[QA_TSC_NUM_EXTRA_REWARDS];   /* rewards.scales.<name> * dt (_prepare_reward_function :1107-1113); 0 = the term is not computed */
    /* dof_acc divides by dt.  This carries the RECIPROCAL, (float)1 / (float)dt, and the kernel multiplies: that is what the reference's
     * `tensor / self.dt` does on its device (torch's division of a device tensor by a host scalar multiplies by the scalar's fp32
     * reciprocal).  torch on the CPU divides instead; the two differ by at most one ulp per joint before the square. */
    float inv_dt;
    float default_dof_pos[12];
    float dof_pos_lower[12], dof_pos_upper[12]; /* the SOFT limits m -+ 0.5 r soft_dof_pos_limit of :613-616 */
    float dof_vel_limit_soft[12];               /* dof_vel_limits * rewards.soft_dof_vel_limit, the fp32 product the reference's tensor * scalar forms */
    float torque_limit_soft[12];                /* torque_limits * rewards.soft_torque_limit, likewise */
    int32_t reserved;
    /* device pointers, all owned by the caller; (N,12) rows and dof_state must be 16-byte aligned (they are read as 16-byte words) */
    const float *dof_state;                     /* (N,12,2) the arena's DOF_STATE: [2k] = position, [2k+1] = velocity of joint k */
    const float *actions;                       /* (N,12) ACTIONS */
    float *prev_actions;                        /* (N,12) read + written: the reference's last_actions, see below */
    const float *torques_org;                   /* (N,12) TORQUES_ORG */
    float *prev_torques_org;                    /* (N,12) read + written: the reference's last_torques_org, see below */
    float *prev_dof_vel;                        /* (N,12) read + written: the reference's last_dof_vel, see below */
    float *extra_episode_sums;                  /* (QA_TSC_NUM_EXTRA_REWARDS, N) read + written, episode_sums' layout */
} qa_tsc_extra_rewards;

/* qa_tsc_goal_step with the terms above whose scale_dt is non-zero.  `extra` == NULL, or every scale_dt zero: exactly
 * qa_tsc_goal_step (the same kernel instantiation, no pointer of `extra` is looked at).  Otherwise
 *   - rew_buf is built in the reference's order (compute_reward :412-430): alphabetical over the 21 non-termination names of BOTH
 *     sets, the eight as qa_tsc_goal_step adds them (term * scale also for a zero scale), an extra term with a zero scale skipped;
 *     then the clip at zero, then `termination`;
 *   - every extra term that is on is added to its row of extra_episode_sums; rows of terms that are off are not touched;
 *   - hip_pos sums joints 0, 3, 6, 9 (the hip of each leg in the engine's joint order);
 *   - feet_stumble tests the feet of cfg->feet_bodies on io->contact_forces;
 *   - prev_dof_vel: dof_acc reads it, and the call ends by storing  prev_dof_vel[e] = reset_buf[e] ? 0 : dof_vel[e]  (only when
 *     dof_acc is on).  That is the reference's last_dof_vel: `dof_vel` as post_physics_step leaves it (:280), i.e. refreshed before
 *     this call, the resetting envs' rows zeroed by _reset_dofs, and NOT read again after reset_idx's extra simulate.  The arena's
 *     LAST_DOF_VEL is the state the next physics launch starts from, which is after that simulate, so it cannot stand in.
 *     A full reset starts the buffer at zero.
 *   - prev_actions / prev_torques_org: action_rate / delta_torques read them, and the call ends by storing  prev_actions[e] = actions[e]
 *     (only when action_rate is on) and  prev_torques_org[e] = torques_org[e]  (only when delta_torques is on), for EVERY env: the
 *     reference copies them at :279 / :281, after reset_idx, so what :387 / :389 zeroed is overwritten.  The arena's LAST_ACTIONS /
 *     LAST_TORQUES_ORG hold the same values while the goal step runs, but the reset that follows zeroes their resetting rows, so after a
 *     step they are not what the reference holds; the owned buffers are.  A full reset starts them at zero.
 * Pointers a term needs: action_rate: actions, prev_actions; delta_torques: torques_org, prev_torques_org; torques, torque_limits:
 * torques_org; dof_acc: dof_state, prev_dof_vel; dof_error, dof_pos_limits, dof_vel_limits, hip_pos: dof_state.  Returns QA_E_ARG
 * when a term that is on lacks one of them or finds it misaligned, when extra_episode_sums is NULL while any term is on, and for
 * everything qa_tsc_goal_step refuses.  Nothing is kept between calls; the launch can be recorded into a hipGraph. */
int qa_tsc_goal_step_rewards(const qa_tsc_goal_cfg *cfg, const qa_tsc_goal_io *io, const qa_tsc_extra_rewards *extra, void *stream);

#ifdef __cplusplus
}
#endif
#endif
