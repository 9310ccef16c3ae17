// qa_tsc_rewards.h -- the arithmetic of the task-level tree's fourteen extra reward terms (include/qa_tsc_rewards.h) and of the
// reference's summation order over all 22, ONCE, for host and device: qa_tsc_goal_step_kernel<true> (qa_tsc.hip) calls these functions
// with values it holds in registers, and the host twin of tests/c_host/qa_tsc_rewards_host.cpp calls the same functions on the fixture
// of tests/golden/tsc_rewards.npz.  Plain floats in, plain floats out; fp32 like the torch tensors of
// tsc/legged_gym/envs/base/legged_robot.py:1824-1925.  A 12-joint row is summed joint 0 .. 11.
#ifndef QA_TSC_REWARDS_IMPL_H
#define QA_TSC_REWARDS_IMPL_H

#include "../../include/qa_tsc_rewards.h"
#include "qa_rewards.h"          // QA_RW_FN, and the terms whose arithmetic the two trees share: lin_vel_z, ang_vel_xy, orientation, feet_stumble

QA_RW_FN float qa_tsc_rw_action_rate(const float *last_actions, const float *actions) {          // :1844  norm, not its square
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) { const float d = last_actions[k] - actions[k]; s += d * d; }
    return sqrtf(s);
}
QA_RW_FN float qa_tsc_rw_delta_torques(const float *torques_org, const float *last_torques_org) { // :1861
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) { const float d = torques_org[k] - last_torques_org[k]; s += d * d; }
    return s;
}
QA_RW_FN float qa_tsc_rw_dof_acc(const float *prev_dof_vel, const float *dof_vel, float inv_dt) {  // :1837
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) { const float a = (prev_dof_vel[k] - dof_vel[k]) * inv_dt; s += a * a; }
    return s;
}
QA_RW_FN float qa_tsc_rw_dof_error(const float *dof_pos, const float *default_dof_pos) {           // :1889
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) { const float d = dof_pos[k] - default_dof_pos[k]; s += d * d; }
    return s;
}
QA_RW_FN float qa_tsc_rw_dof_pos_limits(const float *dof_pos, const float *lower, const float *upper) {   // :1872
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) s += -fminf(dof_pos[k] - lower[k], 0.0f) + fmaxf(dof_pos[k] - upper[k], 0.0f);
    return s;
}
QA_RW_FN float qa_tsc_rw_dof_vel_limits(const float *dof_vel, const float *limit_soft) {           // :1878  clip(0, 1) per joint
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) s += fminf(fmaxf(fabsf(dof_vel[k]) - limit_soft[k], 0.0f), 1.0f);
    return s;
}
QA_RW_FN float qa_tsc_rw_every_step() { return 1.0f; }                                             // :1924
QA_RW_FN float qa_tsc_rw_hip_pos(const float *dof_pos, const float *default_dof_pos) {             // :1885  hip_indices = joints 0, 3, 6, 9
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; k += 3) { const float d = dof_pos[k] - default_dof_pos[k]; s += d * d; }
    return s;
}
QA_RW_FN float qa_tsc_rw_torque_limits(const float *torques_org, const float *limit_soft) {        // :1867
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) s += fmaxf(fabsf(torques_org[k]) - limit_soft[k], 0.0f);
    return s;
}
QA_RW_FN float qa_tsc_rw_torques(const float *torques_org) {                                       // :1864
    float s = 0.0f;
    QA_RW_UNROLL
    for (int k = 0; k < 12; ++k) s += torques_org[k] * torques_org[k];
    return s;
}
// last_dof_vel as :280 leaves it behind reset_idx (include/qa_tsc_rewards.h has the why)
QA_RW_FN float qa_tsc_rw_next_prev_dof_vel(float dof_vel, int reset) { return reset ? 0.0f : dof_vel; }

// compute_reward (:412-430) over both sets.  The reference walks its reward_scales dict, whose keys class_to_dict sorted: alphabetical
// over the seven non-termination names of QA_TSC_REW_* and the fourteen of QA_TSC_XR_*.  Entry >= 0: index into the former, entry < 0:
// ~index into the latter.  `termination` is not in the walk: it is added behind the clip.
#define QA_TSC_RW_WALK 21
QA_RW_FN int qa_tsc_rw_walk(int i) {
    constexpr signed char walk[QA_TSC_RW_WALK] = {
        0 /* action_hl_rate */, ~QA_TSC_XR_ACTION_RATE, ~QA_TSC_XR_ANG_VEL_XY, 1 /* collision */, ~QA_TSC_XR_DELTA_TORQUES, ~QA_TSC_XR_DOF_ACC,
        ~QA_TSC_XR_DOF_ERROR, ~QA_TSC_XR_DOF_POS_LIMITS, ~QA_TSC_XR_DOF_VEL_LIMITS, ~QA_TSC_XR_EVERY_STEP, 2 /* feet_edge */, ~QA_TSC_XR_FEET_STUMBLE,
        ~QA_TSC_XR_HIP_POS, 3 /* latent_c_rate */, ~QA_TSC_XR_LIN_VEL_Z, ~QA_TSC_XR_ORIENTATION, 4 /* reach_goal */, ~QA_TSC_XR_TORQUE_LIMITS,
        ~QA_TSC_XR_TORQUES, 5 /* tracking_goal_vel */, 6 /* tracking_yaw */};
    return walk[i];
}
// term / scale_dt / sums of the eight (b*) and of the fourteen (x*).  A base term is added as qa_tsc_goal_step adds it: term * scale, a
// zero scale included; an extra term with a zero scale is skipped, as the reference drops it (:1107-1113).  The clip is unconditional
// (only_positive_rewards, as in qa_tsc_goal_step).  Returns the step's reward; every sum gains its term.
QA_RW_FN float qa_tsc_rw_total(const float *bterm, const float *bscale, float *bsum, const float *xterm, const float *xscale, float *xsum_) {
    float rew = 0.0f;
    QA_RW_UNROLL
    for (int i = 0; i < QA_TSC_RW_WALK; ++i) {
        const int w = qa_tsc_rw_walk(i);
        if (w >= 0) { const float v = bterm[w] * bscale[w]; rew += v; bsum[w] += v; }
        else { if (xscale[~w] != 0.0f) { const float v = xterm[~w] * xscale[~w]; rew += v; xsum_[~w] += v; } }
    }
    rew = fmaxf(rew, 0.0f);
    const float v = bterm[QA_TSC_REW_TERMINATION] * bscale[QA_TSC_REW_TERMINATION];
    rew += v; bsum[QA_TSC_REW_TERMINATION] += v;
    return rew;
}

#endif
