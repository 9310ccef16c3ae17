/* qa_sim_actuators.h -- extension of include/qa_sim.h: the actuator model of the fused env step -- control.control_type 'P', 'V' or 'T' and
 * one PD gain pair per joint (control.stiffness / control.damping dicts that do not give every joint the same gains).
 *
 * Kept apart from qa_sim.h for the reason qa_sim_rewards.h is: that header is the ABI the CPU oracle twins symbol by symbol
 * (tests/test_abi.py), and this feature adds neither an arena tensor nor a config field to it.  The library exports the entry point next to
 * the ABI; the Python side binds it through _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_SIM_ACTUATORS_H
#define QA_SIM_ACTUATORS_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* control.control_type (bbc/legged_gym/envs/base/legged_robot.py:561-577, tsc/legged_gym/envs/base/legged_robot.py:776-791) */
#define QA_ACTUATOR_P 0
#define QA_ACTUATOR_V 1
#define QA_ACTUATOR_T 2

/* kp[j], kd[j]: the reference's p_gains / d_gains, joint j = 3 * leg + k in the engine's order (FL, FR, RL, RR x hip, thigh, calf). */
typedef struct {
    int32_t control_type;                   /* QA_ACTUATOR_* */
    float kp[QA_NUM_DOF];
    float kd[QA_NUM_DOF];
} qa_actuators;

/* _compute_torques of both trees.  Without this call (and after a call with a NULL struct) the step computes the P law from the ONE gain pair
 * cfg.kp / cfg.kd, as it always did, in the kernels it always ran.  With a struct, qa_env_step / qa_env_step_dev (plane with and without helper
 * wavefronts, height field, every lean mask, with and without the extra reward terms) and qa_env_physics_step run other instantiations of the
 * step kernel, which take the law and the gains from the handle; cfg.kp / cfg.kd are not read.  Per substep, in fp32, every product, sum and
 * quotient rounded on its own and in this order (no contraction), with as = action * cfg.action_scale (* cfg.hip_scale_reduction on the four
 * hip joints), q0 = cfg.default_dof_pos, q / qd the joint's state at the start of the substep:
 *     P   tau = gp * (as + q0 - q) - gd * qd        gp = kp[j], gd = kd[j]; with cfg.randomize_motor gp = strength_p * kp[j] and
 *                                                   gd = strength_d * kd[j], the products the reference forms first (MOTOR_STRENGTH rows 0 / 1)
 *     V   tau = kp[j] * (as - qd) - kd[j] * (qd - last_qd) / cfg.sim_dt      the quotient correctly rounded; the motor strength is not read
 *     T   tau = as                                                           the motor strength is not read
 * last_qd is read ONCE per env step and held over its substeps, as the reference's last_dof_vel is: in qa_env_step / qa_env_step_dev it is the
 * env's row of QA_T_LAST_DOF_VEL as the step finds it (the joint velocities the previous step ended with, zero after a reset); in
 * qa_env_physics_step it is the joint velocity the step starts from, which is what that step writes to QA_T_LAST_DOF_VEL and what the
 * task-level tree's last_dof_vel holds when its _compute_torques runs.  QA_T_LAST_DOF_VEL is updated where it always was.
 * TORQUES_ORG takes tau, TORQUES tau clamped to the URDF effort limits, as before.  qa_simulate / qa_simulate_if take their torques from the
 * caller and are not affected.
 *
 * The actuator instantiations exist without the self-collision rows of include/qa_sim_selfcol.h only: this call returns QA_E_ARG on a handle
 * whose qa_set_self_collision_hips / qa_set_self_collision_thighs is on, and those return QA_E_ARG while an actuator model is set.
 *
 * The struct is copied to a 24-float device table the handle owns (allocated at the first call, released by qa_destroy); the call waits for
 * the device to be idle before it overwrites the table.  So the device the arena lives on must be the CURRENT device of the calling thread
 * (hipSetDevice; the allocation and the copy go to the current device), and the call must not be made while a stream capture is open (the wait
 * fails there and the call returns QA_E_DEVICE).  The choice selects other kernel instantiations at launch time: a recorded rollout
 * (hipGraph) bakes it in.  Call this BEFORE the first recording, and record again after changing it.
 * Returns QA_E_ARG on a NULL handle, on a control_type that is none of QA_ACTUATOR_*, on a gain that is not finite and on the combination with
 * the self-collision levels. */
int qa_set_actuators(qa_sim *sim, const qa_actuators *actuators);

#ifdef __cplusplus
}
#endif
#endif
