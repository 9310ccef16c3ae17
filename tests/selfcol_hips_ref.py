"""float64 reference of the calf-against-neighbouring-hip self-collision class: forward kinematics of the two shapes in the
base frame and a closed-form segment-segment distance.  Shared by tests/test_selfcol_hips_cpu.py, tests/test_selfcol_hips.py and
tools/self_collision_hips_sweep.py; independent of the kernel's code (numpy only).

Shapes, as tools/self_collision_proximity.py::capsules has them for the hip and as csrc/qa_physics.h has them for the calf:
  calf  capsule from the knee to the foot centre (-0.002, 0, -0.213 in the calf frame), radius 13 mm at the knee growing to 22 mm at the foot
  hip   the URDF's hip cylinder as a capsule: (0, +-0.06, 0) .. (0, +-0.10, 0) in the hip link's frame (+ for left legs), radius 46 mm
"""
import numpy as np

LEGS = ("FL", "FR", "RL", "RR")
HIP_ORG = np.array([[0.1934, 0.0465, 0.0], [0.1934, -0.0465, 0.0], [-0.1934, 0.0465, 0.0], [-0.1934, -0.0465, 0.0]])
SIDE = np.array([1.0, -1.0, 1.0, -1.0])
DOF_LOWER = np.array([[-1.0472, -1.5708, -2.7227], [-1.0472, -1.5708, -2.7227], [-1.0472, -0.5236, -2.7227], [-1.0472, -0.5236, -2.7227]])
DOF_UPPER = np.array([[1.0472, 3.4907, -0.83776], [1.0472, 3.4907, -0.83776], [1.0472, 4.5379, -0.83776], [1.0472, 4.5379, -0.83776]])
CALF_R0, CALF_R1, HIP_R = 0.013, 0.022, 0.046
HIP_Y0, HIP_Y1 = 0.06, 0.10
CONTACT_OFFSET = 0.01
# the ordered (calf leg, hip leg) relations of front / rear neighbours.  Only the first two get a row: a front calf reaches the rear hip of
# its side (-68 mm), while every other relation stays >= 24 mm apart under the joint limits (tools/self_collision_hips_sweep.py,
# profiles/self_collision_hips_sweep.json) -- the rear thigh's -0.52 rad lower stop keeps the rear calf off the front hip
ROW_RELATIONS = ((0, 2), (1, 3))
RELATIONS = ((0, 2), (1, 3), (2, 0), (3, 1))


def leg_points(q, leg):
    """q (..., 3) joint angles of leg `leg` -> (knee, foot, hip0, hip1), each (..., 3), base frame, float64"""
    q = np.asarray(q, np.float64)
    s1, c1 = np.sin(q[..., 0]), np.cos(q[..., 0])
    s2, c2 = np.sin(q[..., 1]), np.cos(q[..., 1])
    s23, c23 = np.sin(q[..., 1] + q[..., 2]), np.cos(q[..., 1] + q[..., 2])
    z = np.zeros_like(s1)
    sy = SIDE[leg]
    yax = np.stack([z, c1, s1], -1)                               # Rx(q0) e_y
    hip0 = HIP_ORG[leg] + sy * HIP_Y0 * yax
    hip1 = HIP_ORG[leg] + sy * HIP_Y1 * yax
    o1 = HIP_ORG[leg] + sy * 0.0955 * yax
    # Rx(q0) Ry(t) = [[c, 0, s], [s1 s, c1, -s1 c], [-c1 s, s1, c1 c]]; its third column times -0.213
    col3 = lambda s, c: np.stack([s, -s1 * c, c1 * c], -1)
    col1 = lambda s, c: np.stack([c, s1 * s, -c1 * s], -1)
    knee = o1 - 0.213 * col3(s2, c2)
    foot = knee - 0.002 * col1(s23, c23) - 0.213 * col3(s23, c23)
    return knee, foot, hip0, hip1


def seg_seg(a0, a1, b0, b1):
    """closed-form closest points of segments a0 + s (a1 - a0), b0 + t (b1 - b0) in float64 (batched): returns (dist, s, t).  Exact
    minimisation of the convex quadratic over the unit square: the interior stationary point when it is inside, else the best of the
    four edges (each a point-segment projection)."""
    a0, a1, b0, b1 = (np.asarray(v, np.float64) for v in (a0, a1, b0, b1))
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, f = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d2 * r).sum(-1)
    c, b = (d1 * r).sum(-1), (d1 * d2).sum(-1)
    den = a * e - b * b

    def dist2(s, t):
        v = r + s[..., None] * d1 - t[..., None] * d2
        return (v * v).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        si = np.where(den > 1e-300, (b * f - c * e) / den, 0.0)
        ti = np.where(den > 1e-300, (a * f - b * c) / den, 0.0)
    inside = (den > 1e-300) & (si >= 0) & (si <= 1) & (ti >= 0) & (ti <= 1)
    cands = []
    for sfix in (0.0, 1.0):                                        # edges s = 0, 1: project onto B
        s = np.full_like(a, sfix)
        t = np.clip((b * s + f) / e, 0, 1)
        cands.append((s, t))
    for tfix in (0.0, 1.0):                                        # edges t = 0, 1: project onto A
        t = np.full_like(a, tfix)
        s = np.clip((b * t - c) / a, 0, 1)
        cands.append((s, t))
    best_s, best_t = cands[0]
    best = dist2(best_s, best_t)
    for s, t in cands[1:]:
        d = dist2(s, t)
        m = d < best
        best, best_s, best_t = np.where(m, d, best), np.where(m, s, best_s), np.where(m, t, best_t)
    di = dist2(np.clip(si, 0, 1), np.clip(ti, 0, 1))
    use = inside & (di <= best)
    best, best_s, best_t = np.where(use, di, best), np.where(use, si, best_s), np.where(use, ti, best_t)
    return np.sqrt(best), best_s, best_t


def calf_hip_gap(q_calf, calf_leg, q_hip, hip_leg):
    """gap (m), unit normal hip -> calf, the two segment parameters and the four end points of the ordered relation"""
    knee, foot, _, _ = leg_points(q_calf, calf_leg)
    _, _, h0, h1 = leg_points(q_hip, hip_leg)
    d, s, t = seg_seg(knee, foot, h0, h1)
    pa = knee + s[..., None] * (foot - knee); pb = h0 + t[..., None] * (h1 - h0)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (pa - pb) / d[..., None]
    gap = d - (CALF_R0 + s * (CALF_R1 - CALF_R0)) - HIP_R
    return gap, n, s, t, (knee, foot, h0, h1)


def all_gaps(dof_pos):
    """dof_pos (..., 12) -> (..., 4) gaps of RELATIONS"""
    dof_pos = np.asarray(dof_pos, np.float64)
    return np.stack([calf_hip_gap(dof_pos[..., 3 * a:3 * a + 3], a, dof_pos[..., 3 * b:3 * b + 3], b)[0] for a, b in RELATIONS], -1)
