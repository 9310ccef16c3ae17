"""The Go2's joint limits as its URDF states them, in the engine's joint order (_capi.DOF_NAMES), for both trees' `LeggedRobot`
(`dof_pos_limits`, `dof_vel_limits`, `torque_limits`, `hip_indices` of the reference's _process_dof_props, legged_robot.py:403-430 of the
behaviour-level tree and :596-617 of the task-level one)."""
import torch

DOF_POS_LOWER = [-1.0472, -1.5708, -2.7227] * 2 + [-1.0472, -0.5236, -2.7227] * 2
DOF_POS_UPPER = [1.0472, 3.4907, -0.83776] * 2 + [1.0472, 4.5379, -0.83776] * 2
DOF_VEL_LIMITS = [30.1, 30.1, 20.07] * 4
TORQUE_LIMITS = [20.0, 20.0, 40.0] * 4
HIP_INDICES, THIGH_INDICES, CALF_INDICES = [0, 3, 6, 9], [1, 4, 7, 10], [2, 5, 8, 11]


def soft_dof_pos_limits(soft_dof_pos_limit, device=None):
    """(12, 2) fp32: the soft position limits  m -+ 0.5 r s  around the middle of the URDF range, as the reference forms them"""
    lo = torch.tensor(DOF_POS_LOWER, device=device)
    hi = torch.tensor(DOF_POS_UPPER, device=device)
    m, r = (lo + hi) / 2, hi - lo
    s = soft_dof_pos_limit
    return torch.stack([m - 0.5 * r * s, m + 0.5 * r * s], dim=1)
