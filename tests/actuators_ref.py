"""Float64 restatement of the three actuator laws of include/qa_sim_actuators.h (_compute_torques of both reference trees,
bbc/legged_gym/envs/base/legged_robot.py:559-579): the reference of the GPU tests of tests/test_actuators.py, itself checked against
hand-computed values in tests/test_actuators_cpu.py.  No GPU, no library: numpy only."""
import numpy as np

HIPS = [0, 3, 6, 9]
FP32_ROUNDING = 2.0 ** -24            # one rounding to nearest: at most this times the magnitude of the value rounded


def clip_actions(actions, clip, action_scale):
    """legged_robot.py:96-98, in fp32 as the step does it"""
    lim = np.float32(clip) / np.float32(action_scale)
    return np.clip(np.asarray(actions, np.float32), -lim, lim)


def scaled_actions(actions, action_scale, hip_scale_reduction):
    a = np.asarray(actions, np.float64) * float(action_scale)
    a[..., HIPS] *= float(hip_scale_reduction)
    return a


def torques(control_type, actions, q, qd, last_qd, kp, kd, q0, action_scale, hip_scale_reduction, sim_dt, strength=None):
    """(tau_org, largest) in float64 for (N, 12) clipped actions and joint state: the unclipped torque of the law, and per element the largest
    magnitude among the intermediates met while evaluating it (what an fp32 evaluation's roundings are relative to).
    strength: (2, N, 12) motor strength for the P law with randomize_motor, None without; V and T ignore it, as the reference does."""
    f = lambda x: np.asarray(x, np.float64)
    a_s, q, qd, last_qd, kp, kd, q0 = scaled_actions(actions, action_scale, hip_scale_reduction), f(q), f(qd), f(last_qd), f(kp), f(kd), f(q0)
    if control_type == "T":
        return a_s, np.abs(a_s)
    if control_type == "V":
        e, dv = a_s - qd, qd - last_qd
        t1, x = kp * e, kd * dv
        t2 = x / float(sim_dt)
        tau = t1 - t2
        parts = (a_s, qd, e, t1, dv, x, t2, tau)
    elif control_type == "P":
        gp, gd = (kp, kd) if strength is None else (f(strength[0]) * kp, f(strength[1]) * kd)
        s1 = a_s + q0
        e = s1 - q
        t1, t2 = gp * e, gd * qd
        tau = t1 - t2
        parts = (a_s, s1, e, t1, t2, tau, gp + 0 * tau, gd + 0 * tau)
    else:
        raise NameError(f"Unknown controller type: {control_type}")
    return tau, np.max(np.abs(np.stack(np.broadcast_arrays(*parts))), axis=0)


def clamp(tau, limits):
    limits = np.asarray(limits, np.float64)
    return np.clip(tau, -limits, limits)


def state_coefficients(control_type, kp, kd, sim_dt):
    """(|d tau / d q|, |d tau / d qd|) per joint: how an error of the state the substep starts from reaches the torque"""
    kp, kd = np.abs(np.asarray(kp, np.float64)), np.abs(np.asarray(kd, np.float64))
    if control_type == "T":
        return 0 * kp, 0 * kp
    if control_type == "V":
        return 0 * kp, kp + kd / float(sim_dt)
    return kp, kd
