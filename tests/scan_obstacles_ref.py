"""Float64 statement of the height scan on the articulated obstacles' rendered surface (include/qa_tsc_scan_obstacles.h): the static scan of
qa_tsc_observations -- the 132 grid points turned by the trunk's yaw alone, the lowest of three map samples per point -- and, on top of it,
tests/depth_obstacles_ref.py's footprint test and surface.  Not the oracle: the oracle has no twin of the obstacle entry point."""
import numpy as np

from tests import depth_obstacles_ref as dref

NUM_SCAN, CENTRE = 132, 67                            # QA_TSC_NUM_SCAN and the point the root height reads (NUM_SCAN / 2 + 1)
OFF_SCAN, OFF_ROOT_H, BBC_ROOT_H, DISC_ROOT_H = 65, 197, 57, 2
EDGE = 1e-3                                           # m: a point nearer than this to a footprint edge or to the plank's ground line may flip


def world_points(root, points):
    """(132,) world x and y of one env's scan points: quat_apply of the yaw-only quaternion (0, 0, q2, q3) / |(q2, q3)|, plus the root"""
    root, points = np.asarray(root, np.float64), np.asarray(points, np.float64)
    qn = max(np.hypot(root[5], root[6]), 1e-9)
    qz, qw = root[5] / qn, root[6] / qn
    bx, by = points[:, 0], points[:, 1]
    t0, t1 = -qz * by * 2.0, qz * bx * 2.0
    return bx + qw * t0 - qz * t1 + root[0], by + qw * t1 + qz * t0 + root[1]


def static_heights(hmap, x, y, border, hs, vs):
    """_get_heights (legged_robot.py:1708-1755): the lowest of the samples (px, py), (px + 1, py), (px, py + 1)"""
    hmap = np.asarray(hmap)
    rows, cols = hmap.shape
    px = np.clip(((x + border) / hs).astype(np.int64), 0, rows - 2); py = np.clip(((y + border) / hs).astype(np.int64), 0, cols - 2)
    return vs * np.minimum(np.minimum(hmap[px, py], hmap[px + 1, py]), hmap[px, py + 1]).astype(np.float64)


def edge_distance(rec, x, y):
    """distance of (x, y) to the border of the nearest non-empty slot's footprint, from inside or from outside"""
    d = np.full(np.shape(x), np.inf)
    for k in range(3):
        r = rec[k]
        if r[7] == 0.0:
            continue
        dx, dy = x - r[0], y - r[1]
        a, b = np.abs(r[2] * dx + r[3] * dy) - r[4], np.abs(r[2] * dy - r[3] * dx) - r[5]
        d = np.minimum(d, np.where((a <= 0) & (b <= 0), np.minimum(-a, -b), np.hypot(np.maximum(a, 0.0), np.maximum(b, 0.0))))
    return d


def scan(root, points, hmap, desc, state, border=5.0, hs=0.05, vs=0.005):
    """one env: dict of (132,) arrays -- x, y; mode (0 none, 1 see-saw, 2 bar / tyre), q of the covering slot; `static`, the map's height;
    `height`, the measured one; `doubtful`, the points the comparison may leave out (EDGE)"""
    rec = dref.records(desc, state)
    x, y = world_points(root, points)
    static = static_heights(hmap, x, y, border, hs, vs)
    mode, lx, slot = dref.classify(rec, x, y)
    k = np.maximum(slot, 0)
    height = dref.surface(rec, x, y, static, static)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ground_line = np.where((mode == 1) & (rec[k, 10] != 0.0), np.abs(lx - rec[k, 6] / rec[k, 10]), np.inf)      # where h0 - lx tan q = 0
    doubtful = (edge_distance(rec, x, y) < EDGE) | (ground_line < EDGE)
    return dict(x=x, y=y, mode=mode, q=np.where(mode != 0, rec[k, 8], 0.0), lx=lx, static=static, height=height, doubtful=doubtful)


def tolerance(x, y):
    """8 fp32 roundings of the point's world coordinates (tests/test_depth_obstacles_cpu.py holds the host twin of the surface to the same)"""
    return 8.0 * 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(x), np.abs(y)))
