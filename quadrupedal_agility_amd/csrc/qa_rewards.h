// qa_rewards.h -- the arithmetic of the extra reward terms (include/qa_sim_rewards.h) and of the reference's summation order, ONCE, for
// host and device: post_physics_phase (qa_sim.hip) calls these functions with values it holds in registers, and the host twin of
// tests/c_host/qa_extra_rewards_host.cpp calls the same functions on the fixtures of tests/golden/extra_rewards.npz.  Plain floats in,
// plain floats out; fp32 like the torch tensors of bbc/legged_gym/envs/base/legged_robot.py:1231-1365.  "_leg" functions are the share
// of one leg (one lane of the env's quad); the caller adds the four shares.
#ifndef QA_REWARDS_H
#define QA_REWARDS_H

#include <math.h>

#include "../../include/qa_sim_rewards.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QA_RW_FN __host__ __device__ __forceinline__
#define QA_RW_UNROLL _Pragma("unroll")
#else
#define QA_RW_FN static inline
#define QA_RW_UNROLL
#endif

QA_RW_FN float qa_rw_lin_vel_z(float vz) { return vz * vz; }                                   // :1231
QA_RW_FN float qa_rw_ang_vel_xy(float wx, float wy) { return wx * wx + wy * wy; }                // :1235
QA_RW_FN float qa_rw_orientation(float gx, float gy) { return gx * gx + gy * gy; }               // :1239
// :1243  mean_height = mean over the scan of (root z - measured height)
QA_RW_FN float qa_rw_base_height(float mean_height, float target) { const float d = mean_height - target; return d * d; }
QA_RW_FN float qa_rw_dof_vel_leg(float qd0, float qd1, float qd2) { return qd0 * qd0 + qd1 * qd1 + qd2 * qd2; }     // :1263
QA_RW_FN float qa_rw_command_norm(float cx, float cy) { return sqrtf(cx * cx + cy * cy); }
// :1337-1349 for one foot.  contact_z = foot force z > 1, contact = |foot force| > 2 (what post_physics_step has just written to
// last_contacts, :144-146).  Advances *air_time; returns the foot's share of the sum of :1345.  The caller multiplies the sum by
// qa_rw_moving() and stores contact_z as the new last_contacts.
QA_RW_FN float qa_rw_feet_air_time_leg(float *air_time, bool contact_z, bool contact, float dt) {
    const bool filt = contact_z || contact;
    const float first = (*air_time > 0.0f && filt) ? 1.0f : 0.0f;
    const float t = *air_time + dt;
    *air_time = filt ? 0.0f : t;
    return (t - 0.5f) * first;
}
QA_RW_FN float qa_rw_moving(float command_norm) { return command_norm > 0.1f ? 1.0f : 0.0f; }     // :1347
QA_RW_FN int qa_rw_feet_stumble_leg(float fx, float fy, float fz) { return sqrtf(fx * fx + fy * fy) > 4.0f * fabsf(fz) ? 1 : 0; }   // :1351, any() over the feet
QA_RW_FN float qa_rw_stand_still_leg(float q0, float q1, float q2, float d0, float d1, float d2) { return fabsf(q0 - d0) + fabsf(q1 - d1) + fabsf(q2 - d2); }
QA_RW_FN float qa_rw_standing(float command_norm) { return command_norm < 0.1f ? 1.0f : 0.0f; }   // :1359-1360
QA_RW_FN float qa_rw_feet_contact_forces_leg(float fx, float fy, float fz, float max_force) {      // :1362
    return fmaxf(sqrtf(fx * fx + fy * fy + fz * fz) - max_force, 0.0f);
}
QA_RW_FN float qa_rw_termination(int reset, int time_out) { return (reset && !time_out) ? 1.0f : 0.0f; }   // :1280

// compute_reward (:242-259) over both sets.  The reference walks its reward_scales dict, whose keys class_to_dict sorted: alphabetical
// over the names of the 14 terms of qa_config.reward_scale_dt and of the ten of qa_extra_rewards.scale_dt.  Entry >= 0: index into the
// former (QA_R_*), entry < 0: ~index into the latter (QA_XR_*).  `termination` is not in the walk: it is added behind the clip.
#define QA_RW_WALK 23
QA_RW_FN int qa_rw_walk(int i) {
    constexpr signed char walk[QA_RW_WALK] = {
        0 /* action_rate */, ~QA_XR_ANG_VEL_XY, ~QA_XR_BASE_HEIGHT, 1 /* collision */, 2 /* delta_torques */, 3 /* dof_acc */, 4 /* dof_error */,
        5 /* dof_pos_limits */, ~QA_XR_DOF_VEL, 6 /* dof_vel_limits */, ~QA_XR_FEET_AIR_TIME, ~QA_XR_FEET_CONTACT_FORCES, ~QA_XR_FEET_STUMBLE,
        7 /* hip_pos */, 8 /* jump_up_height */, ~QA_XR_LIN_VEL_Z, 9 /* locomotion_height */, ~QA_XR_ORIENTATION, ~QA_XR_STAND_STILL,
        10 /* torque_limits */, 11 /* torques */, 12 /* tracking_ang_vel */, 13 /* tracking_lin_vel */};
    return walk[i];
}
// term / scale_dt / sums of the 14 (b*) and of the ten (x*); a zero scale skips its term as the reference drops it (:927-930).
// Returns the step's reward; every sum gains its term.
QA_RW_FN float qa_rw_total(const float *bterm, const float *bscale, float *bsum, const float *xterm, const float *xscale, float *xsum_, int only_positive) {
    float rew = 0.0f;
    QA_RW_UNROLL
    for (int i = 0; i < QA_RW_WALK; ++i) {
        const int w = qa_rw_walk(i);
        if (w >= 0) { if (bscale[w] != 0.0f) { const float v = bterm[w] * bscale[w]; rew += v; bsum[w] += v; } }
        else { if (xscale[~w] != 0.0f) { const float v = xterm[~w] * xscale[~w]; rew += v; xsum_[~w] += v; } }
    }
    if (only_positive) rew = fmaxf(rew, 0.0f);
    if (xscale[QA_XR_TERMINATION] != 0.0f) { const float v = xterm[QA_XR_TERMINATION] * xscale[QA_XR_TERMINATION]; rew += v; xsum_[QA_XR_TERMINATION] += v; }
    return rew;
}

#endif
