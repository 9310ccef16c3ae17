"""float64 reference of the calf-against-neighbouring-thigh self-collision class: forward kinematics of the thigh capsule in the
base frame and the gap of an ordered (calf leg, thigh leg) relation.  Shared by tests/test_selfcol_thighs_cpu.py and tests/test_selfcol_thighs.py;
independent of the kernel's header (numpy only; forward kinematics of the calf and the segment-segment closed form come from
tests/selfcol_hips_ref.py).

Shapes:
  calf   capsule from the knee to the foot centre, radius 13 mm at the knee growing to 22 mm at the foot (as for the other two classes)
  thigh  the URDF's thigh box 0.11 x 0.0245 x 0.034 as its circumscribed capsule, as tools/self_collision_proximity.py::capsules has it:
         segment (0, 0, -0.0515) .. (0, 0, -0.1615) in the thigh link's frame, radius 21 mm
"""
import numpy as np

from tests.selfcol_hips_ref import CALF_R0, CALF_R1, CONTACT_OFFSET, DOF_LOWER, DOF_UPPER, HIP_ORG, LEGS, SIDE, leg_points, seg_seg  # noqa: F401

THIGH_R = 0.021
THIGH_Z0, THIGH_Z1 = -0.0515, -0.1615
# the ordered (calf leg, thigh leg) relations that get a row: front / rear neighbours of the same side, both orderings
ROW_RELATIONS = ((0, 2), (2, 0), (1, 3), (3, 1))
# the two isolated example poses: a calf 40 mm inside the other leg's thigh with every calf-calf, calf-hip and reverse calf-thigh gap of the
# pair above 20 mm -- (calf leg, its joints, thigh leg, its joints)
EXAMPLES = ((0, (-0.50, 1.73, -1.14), 2, (-0.50, -0.39, -1.01)),
            (2, (0.42, -0.49, -1.80), 0, (-0.47, 1.92, -1.15)))


def thigh_points(q, leg):
    """q (..., 3) joint angles of leg `leg` -> (thigh joint origin, t0, t1), each (..., 3), base frame, float64"""
    q = np.asarray(q, np.float64)
    s1, c1 = np.sin(q[..., 0]), np.cos(q[..., 0])
    s2, c2 = np.sin(q[..., 1]), np.cos(q[..., 1])
    z = np.zeros_like(s1)
    o1 = HIP_ORG[leg] + SIDE[leg] * 0.0955 * np.stack([z, c1, s1], -1)
    zax = np.stack([s2, -s1 * c2, c1 * c2], -1)                    # Rx(q0) Ry(q1) e_z
    return o1, o1 + THIGH_Z0 * zax, o1 + THIGH_Z1 * zax


def calf_thigh_gap(q_calf, calf_leg, q_thigh, thigh_leg):
    """gap (m), unit normal thigh -> calf, the two segment parameters and the four end points of the ordered relation"""
    knee, foot, _, _ = leg_points(q_calf, calf_leg)
    _, t0, t1 = thigh_points(q_thigh, thigh_leg)
    d, s, t = seg_seg(knee, foot, t0, t1)
    pa = knee + s[..., None] * (foot - knee); pb = t0 + t[..., None] * (t1 - t0)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (pa - pb) / d[..., None]
    gap = d - (CALF_R0 + s * (CALF_R1 - CALF_R0)) - THIGH_R
    return gap, n, s, t, (knee, foot, t0, t1)


def mirror(leg, q):
    """the same pose on the other side of the robot: leg index with left / right swapped, hip roll negated"""
    return leg ^ 1, (-q[0], q[1], q[2])


def all_gaps(dof_pos):
    """dof_pos (..., 12) -> (..., 4) gaps of ROW_RELATIONS"""
    dof_pos = np.asarray(dof_pos, np.float64)
    return np.stack([calf_thigh_gap(dof_pos[..., 3 * a:3 * a + 3], a, dof_pos[..., 3 * b:3 * b + 3], b)[0] for a, b in ROW_RELATIONS], -1)


def calf_calf_gap(qa, a, qb, b):
    """gap of the calf capsules of legs a and b (the modelled calf-calf class), float64"""
    ka, fa, _, _ = leg_points(qa, a)
    kb, fb, _, _ = leg_points(qb, b)
    d, s, t = seg_seg(ka, fa, kb, fb)
    return d - (CALF_R0 + s * (CALF_R1 - CALF_R0)) - (CALF_R0 + t * (CALF_R1 - CALF_R0))
