/* qa_sim_rewards.h -- extension of include/qa_sim.h: ten more of LeggedRobot's reward terms inside the fused env step.
 *
 * Kept apart from qa_sim.h for the reason qa_sim_curriculum.h is: that header is the ABI the CPU oracle twins symbol by symbol
 * (tests/test_abi.py), and this feature adds neither an arena tensor nor a config field nor a reward slot (QA_NUM_REWARDS) to it.
 * The library exports the entry point next to the ABI; the Python side binds it through _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_SIM_REWARDS_H
#define QA_SIM_REWARDS_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The terms, in alphabetical order (bbc/legged_gym/envs/base/legged_robot.py, the line of each _reward_* function):
 *   ang_vel_xy :1235, base_height :1243, dof_vel :1263, feet_air_time :1337-1349, feet_contact_forces :1362, feet_stumble :1351,
 *   lin_vel_z :1231, orientation :1239, stand_still :1357, termination :1280.
 * Not here, and refused by the config translation: contact_force_balance (:1367 reads a 100-step x 4-foot force history per env) and
 * contact_balance (a scale without a function in the reference). */
#define QA_NUM_EXTRA_REWARDS 10
enum {
    QA_XR_ANG_VEL_XY = 0, QA_XR_BASE_HEIGHT, QA_XR_DOF_VEL, QA_XR_FEET_AIR_TIME, QA_XR_FEET_CONTACT_FORCES, QA_XR_FEET_STUMBLE,
    QA_XR_LIN_VEL_Z, QA_XR_ORIENTATION, QA_XR_STAND_STILL, QA_XR_TERMINATION
};
#define QA_MAX_SCAN_POINTS 1024

typedef struct qa_extra_rewards {
    float scale_dt[QA_NUM_EXTRA_REWARDS];   /* rewards.scales.<name> * dt (legged_robot.py:927-932); 0 = the term is not computed */
    float base_height_target;               /* rewards.base_height_target */
    float max_contact_force;                /* rewards.max_contact_force */
    float step_dt;                          /* decimation * sim dt as ONE fp32 value: what `feet_air_time += self.dt` adds (:1344) */
    int32_t num_scan_points;                /* 0: measured_heights = 0 (plane, or terrain.measure_heights off); else <= QA_MAX_SCAN_POINTS */
    const float *scan_offsets;              /* (num_scan_points, 2) device: (x, y) of the measured_points grid in the base's yaw frame (:1174-1188) */
    float *extra_episode_sums;              /* (QA_NUM_EXTRA_REWARDS, N) device, read + written: the running sums, EPISODE_SUMS' layout */
    float *feet_air_time;                   /* (N, 4) device, read + written */
    float *extra_episode_stats;             /* (2, 16) device: per step parity, the sums of the envs that reset (slot 14: their count), as EPISODE_STATS */
} qa_extra_rewards;

/* From now on the reward phase of the fused step (qa_env_step / qa_env_step_dev) and of qa_debug_post_physics, on plane and
 * height-field handles, also evaluates the terms above whose scale_dt is non-zero, and
 *   - builds REW in the reference's order (compute_reward, :242-259): alphabetical over the non-zero terms of BOTH sets, then the
 *     only_positive_rewards clip, then `termination` = reset and not time_out;
 *   - adds every term to its row of extra_episode_sums; an env that resets adds its rows to extra_episode_stats[step & 1] and
 *     zeroes them together with its feet_air_time row (reset_idx :224, :231-234); qa_reset_all zeroes both for every env;
 *   - base_height: mean over the scan points of ROOT z - height (the min-of-three lookup of :1215-1228 on HEIGHT_SAMPLES, the
 *     points split over the env's four lanes), squared distance to base_height_target; with num_scan_points == 0 the scan is 0;
 *   - feet_air_time, when and only when its scale is non-zero, carries the reference's side effect: LAST_CONTACTS is written
 *     with (foot force z > 1) instead of (|foot force| > 2), which changes the next step's CONTACT_FILT (:1340-1342).
 * With all ten scales zero REW, EPISODE_SUMS and every other arena tensor are bit-identical to the feature being off.
 *
 * The buffers are device memory OWNED BY THE CALLER, contiguous, alive for as long as the handle steps with them; the handle keeps
 * the pointers and the scalars, and they travel in the launch arguments of the step.  A recorded rollout (hipGraph) bakes them in:
 * call this BEFORE the first recording, and record again after changing anything.  A NULL struct switches the feature off again.
 * Returns QA_E_ARG on a mix of NULL and non-NULL buffers (scan_offsets must be non-NULL exactly when num_scan_points > 0), on
 * num_scan_points outside [0, QA_MAX_SCAN_POINTS], and on num_scan_points > 0 against a plane handle (terrain_type != 1). */
int qa_set_extra_rewards(qa_sim *sim, const qa_extra_rewards *extra);

#ifdef __cplusplus
}
#endif
#endif
