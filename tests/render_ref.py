"""Float64 reference of the frame renderer (include/qa_render.h, csrc/qa_render.hip): the same scene definition, written independently in
numpy -- the primitive table's VALUES (read from the library or the host twin), world transforms from a body-state array, textbook
closed-form intersections, the two-triangle height surface intersected exactly piece by piece (every lattice line the ray crosses is a
breakpoint; nothing is marched), shading and shadows -- plus the classification of EDGE pixels: a pixel is an edge pixel if any of the four
rays through (centre +- 0.01 pixel in x, centre +- 0.01 pixel in y) gives another id or another shadow state than the centre ray."""
import numpy as np

SPHERE, CAPSULE, BOX = 0, 1, 2
ID_GROUND, ID_CEILING, ID_SKY = 19, 20, -1
CLS_GROUND, CLS_CEILING, CLS_SKY = 5, 6, 7
AMBIENT, CHECKER_SIZE, CHECKER_DARK = 0.35, 0.5, 0.8
NO_CEILING = 32767
FLAG_SHADOWS, FLAG_CHECKER = 1, 2
EDGE_EPS = 0.01
INF = np.inf


def quat_matrix(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def world_prims(rows, table):
    """rows (19,13): the env's body state; table: list of dicts kind / body / cls / a / b / r (body frame)"""
    out = []
    rows = np.asarray(rows, np.float64)
    for p in table:
        r = rows[p["body"]]
        R = quat_matrix(r[3:7])
        w = dict(kind=p["kind"], body=p["body"], cls=p["cls"], r=float(p["r"]), R=R, a=r[:3] + R @ np.asarray(p["a"], np.float64))
        w["b"] = r[:3] + R @ np.asarray(p["b"], np.float64) if p["kind"] == CAPSULE else np.asarray(p["b"], np.float64)
        out.append(w)
    return out


# ------------------------------------------------------------------ intersections: o (M,3) or (3,), d (M,3) unit; t = inf on a miss
def _rows(o, d):
    d = np.asarray(d, np.float64).reshape(-1, 3)
    return np.broadcast_to(np.asarray(o, np.float64), d.shape), d


def ray_sphere(o, d, c, r):
    o, d = _rows(o, d)
    oc = o - c
    dd = np.einsum("ij,ij->i", d, d)                  # the general quadratic: an fp32 direction is unit only up to its rounding
    b = np.einsum("ij,ij->i", oc, d)
    cc = np.einsum("ij,ij->i", oc, oc) - r * r
    disc = b * b - dd * cc
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(np.where(disc > 0, disc, np.nan))) / dd
    ok = (disc > 0) & (cc > 0) & (t > 0)
    t = np.where(ok, t, INF)
    n = (oc + np.where(ok, t, 0.0)[:, None] * d) / r
    return t, n


def ray_capsule(o, d, a, b, r):
    o, d = _rows(o, d)
    ba, oa = b - a, o - a
    baba = ba @ ba
    bard, baoa = d @ ba, oa @ ba
    rdoa, oaoa = np.einsum("ij,ij->i", d, oa), np.einsum("ij,ij->i", oa, oa)
    # the start's distance from the segment
    s = np.clip(baoa / baba, 0.0, 1.0)
    q = oa - s[:, None] * ba
    outside = np.einsum("ij,ij->i", q, q) > r * r
    A = baba * np.einsum("ij,ij->i", d, d) - bard * bard
    B = baba * rdoa - baoa * bard
    Cc = baba * oaoa - baoa * baoa - r * r * baba
    h = B * B - A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        tb = (-B - np.sqrt(np.where(h > 0, h, np.nan))) / A
        y = baoa + tb * bard
    ok = (A > 1e-14 * baba) & (h > 0) & (tb > 0) & (y > 0) & (y < baba)
    tb = np.where(ok, tb, INF)
    tbs = np.where(ok, tb, 0.0)
    nb = (oa + tbs[:, None] * d - (np.where(ok, y, 0.0) / baba)[:, None] * ba) / r
    t1, n1 = ray_sphere(o, d, a, r)
    t2, n2 = ray_sphere(o, d, b, r)
    t = np.minimum(tb, np.minimum(t1, t2))
    n = np.where((tb <= t)[:, None], nb, np.where((t1 <= t2)[:, None], n1, n2))
    t = np.where(outside, t, INF)
    return t, n


def ray_box(o, d, c, R, h):
    o, d = _rows(o, d)
    ol, dl = (o - c) @ R, d @ R                      # body-frame components: columns of R are the axes
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - ol) / dl, (h - ol) / dl
    tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
    par = dl == 0
    inside = np.abs(ol) < h
    tn = np.where(par, np.where(inside, -INF, INF), tn)
    tf = np.where(par, np.where(inside, INF, -INF), tf)
    axis = np.argmax(tn, axis=1)
    tmin, tmax = tn.max(axis=1), tf.min(axis=1)
    ok = (tmin < tmax) & (tmin > 0)
    sgn = -np.sign(np.take_along_axis(dl, axis[:, None], 1)[:, 0])
    n = sgn[:, None] * R.T[axis]
    return np.where(ok, tmin, INF), n


def ray_prim(o, d, w):
    if w["kind"] == SPHERE:
        return ray_sphere(o, d, w["a"], w["r"])
    if w["kind"] == CAPSULE:
        return ray_capsule(o, d, w["a"], w["b"], w["r"])
    return ray_box(o, d, w["a"], w["R"], w["b"])


def robot_hit(o, d, prims):
    o, d = _rows(o, d)
    t = np.full(d.shape[0], INF); n = np.zeros_like(d); idx = np.full(d.shape[0], -1)
    for i, w in enumerate(prims):
        ti, ni = ray_prim(o, d, w)
        better = ti < t
        t = np.where(better, ti, t); n = np.where(better[:, None], ni, n); idx = np.where(better, i, idx)
    return t, n, idx


# ------------------------------------------------------------------ camera
def camera_rays(cam, width, height, dx=0.0, dy=0.0):
    cam = np.asarray(cam, np.float64)
    o = cam[:3]
    f = cam[3:6] - o
    f = f / np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    if r @ r < 1e-12:
        r = np.cross(f, [1.0, 0.0, 0.0])
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    tv = np.tan(0.5 * cam[6]); th = tv * width / height
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    sx = ((j + 0.5 + dx) / width * 2 - 1) * th
    sy = (1 - (i + 0.5 + dy) / height * 2) * tv
    d = f[None, None] + sx[..., None] * r + sy[..., None] * u
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return o, d.reshape(-1, 3)


# ------------------------------------------------------------------ height field: exact, piece by piece
def _pieces(m, vs, fxm, fym):
    rows, cols = m.shape
    ix = np.clip(np.floor(fxm), 0, rows - 2).astype(np.int64); iy = np.clip(np.floor(fym), 0, cols - 2).astype(np.int64)
    u, v = np.clip(fxm - ix, 0, 1), np.clip(fym - iy, 0, 1)
    lower = u >= v
    s00, s11 = m[ix, iy].astype(np.int64), m[ix + 1, iy + 1].astype(np.int64)
    sm = np.where(lower, m[ix + 1, iy], m[ix, iy + 1]).astype(np.int64)
    exists = (s00 != NO_CEILING) & (s11 != NO_CEILING) & (sm != NO_CEILING)
    return ix, iy, lower, exists, vs * s00, vs * sm, vs * s11


def _height(p, fx, fy):
    ix, iy, lower, _, h00, hm, h11 = p
    u, v = np.clip(fx - ix, 0, 1), np.clip(fy - iy, 0, 1)
    a, b = np.where(lower, u, v), np.where(lower, v, u)
    return h00 + a * (hm - h00) + b * (h11 - hm)


def _normal(p, fxm, fym, shape, hs):
    _, _, lower, _, h00, hm, h11 = p
    gu, gv = np.where(lower, hm - h00, h11 - hm), np.where(lower, h11 - hm, hm - h00)
    gu = np.where((fxm < 0) | (fxm > shape[0] - 1), 0.0, gu); gv = np.where((fym < 0) | (fym > shape[1] - 1), 0.0, gv)
    n = np.stack([-gu / hs, -gv / hs, np.ones_like(gu)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _breaks(f0, df, tend, kmax):
    """t at which f0 + t df crosses an integer, t in (0, tend]; (M, kmax) padded with inf"""
    k = np.arange(kmax)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(df > 0, np.floor(f0) + 1, np.ceil(f0) - 1)
        t = (first[:, None] + np.sign(df)[:, None] * k - f0[:, None]) / df[:, None]
    t = np.where((df[:, None] != 0) & (t > 0) & (t <= tend[:, None]), t, INF)
    return t


def heightfield_hit(o, d, terrain, tend):
    """first crossing of the floor surface (from above) or of an existing ceiling triangle (either way) on (0, tend]: t, normal, id"""
    o, d = _rows(o, d)
    hm, cm = terrain["height_samples"], terrain.get("ceiling_samples")
    hs, vs, border = float(terrain["horizontal_scale"]), float(terrain["vertical_scale"]), float(terrain["border_size"])
    M = d.shape[0]
    fx0, fy0 = (o[:, 0] + border) / hs, (o[:, 1] + border) / hs
    dfx, dfy = d[:, 0] / hs, d[:, 1] / hs
    tend = np.broadcast_to(np.asarray(tend, np.float64), (M,))
    span = float(np.max(tend))
    kmax = int(np.ceil(span * max(np.abs(dfx).max(), np.abs(dfy).max(), np.abs(dfx - dfy).max()))) + 3
    T = np.concatenate([np.zeros((M, 1)), _breaks(fx0, dfx, tend, kmax), _breaks(fy0, dfy, tend, kmax), _breaks(fx0 - fy0, dfx - dfy, tend, kmax),
                        tend[:, None]], axis=1)
    T.sort(axis=1)
    ta, tb = T[:, :-1], T[:, 1:]
    valid = np.isfinite(tb) & (tb > ta)
    ta = np.where(valid, ta, 0.0); tb = np.where(valid, tb, 0.0)
    tm = 0.5 * (ta + tb)
    fx = lambda t: fx0[:, None] + t * dfx[:, None]
    fy = lambda t: fy0[:, None] + t * dfy[:, None]
    z = lambda t: o[:, 2:3] + t * d[:, 2:3]
    pf = _pieces(hm, vs, fx(tm), fy(tm))
    ga, gb = z(ta) - _height(pf, fx(ta), fy(ta)), z(tb) - _height(pf, fx(tb), fy(tb))
    hitf = valid & (ga >= 0) & (gb < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(hitf, ta + (tb - ta) * ga / (ga - gb), INF)
    tc = np.full_like(tf, INF); below = np.zeros(tf.shape, bool)
    if cm is not None:
        pc = _pieces(cm, vs, fx(tm), fy(tm))
        ha, hb = z(ta) - _height(pc, fx(ta), fy(ta)), z(tb) - _height(pc, fx(tb), fy(tb))
        hitc = valid & pc[3] & ((ha < 0) != (hb < 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            tc = np.where(hitc, ta + (tb - ta) * ha / (ha - hb), INF)
        below = ha < 0
    th = np.minimum(tf, tc)
    anyhit = np.isfinite(th)
    first = np.argmax(anyhit, axis=1)
    rr = np.arange(M)
    t = np.where(anyhit.any(axis=1), th[rr, first], INF)
    is_ceiling = (tc[rr, first] < tf[rr, first])
    nf = _normal(pf, fx(tm), fy(tm), hm.shape, hs)[rr, first]
    n = nf
    if cm is not None:
        ncm = _normal(pc, fx(tm), fy(tm), cm.shape, hs)[rr, first]
        ncm = np.where(below[rr, first][:, None], -ncm, ncm)
        n = np.where(is_ceiling[:, None], ncm, nf)
    ident = np.where(np.isfinite(t), np.where(is_ceiling, ID_CEILING, ID_GROUND), ID_SKY)
    return t, n, ident


# ------------------------------------------------------------------ the image
def trace(scene, k, dx=0.0, dy=0.0):
    """camera k of the scene: dict(ids, depth, rgb (float, before rounding), shadow) as flat (H*W) arrays"""
    W, H, far = scene["width"], scene["height"], float(scene["far"])
    e = int(scene["env_ids"][k])
    prims = world_prims(scene["body_state"][e], scene["table"])
    pal = np.asarray(scene["palette"], np.float64)
    light = np.asarray(scene["light_dir"], np.float64); light = light / np.linalg.norm(light)
    flags = int(scene.get("flags", FLAG_SHADOWS | FLAG_CHECKER))
    o, d = camera_rays(scene["cameras"][k], W, H, dx, dy)
    t, n, pidx = robot_hit(o, d, prims)
    hit = t < far
    t = np.where(hit, t, far)
    ids = np.where(hit, np.array([p["body"] for p in prims] + [0])[pidx], ID_SKY)
    cls = np.where(hit, np.array([p["cls"] for p in prims] + [0])[pidx], CLS_SKY)
    terrain = scene.get("terrain")
    if terrain is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            tg = np.where((d[:, 2] < 0) & (o[2] > 0), -o[2] / d[:, 2], INF)
        ng = np.broadcast_to([0.0, 0.0, 1.0], d.shape); idg = np.full(d.shape[0], ID_GROUND)
    else:
        tg, ng, idg = heightfield_hit(o, d, terrain, t)
    g = tg < t
    t = np.where(g, tg, t); n = np.where(g[:, None], ng, n); ids = np.where(g, idg, ids)
    cls = np.where(g, np.where(idg == ID_CEILING, CLS_CEILING, CLS_GROUND), cls)
    hp = o + t[:, None] * d
    lam = np.maximum(n @ light, 0.0)
    col = pal[cls].copy()
    ground = ids == ID_GROUND
    if flags & FLAG_CHECKER:
        odd = ((np.floor(hp[:, 0] / CHECKER_SIZE) + np.floor(hp[:, 1] / CHECKER_SIZE)).astype(np.int64) & 1) == 1
        col = np.where((ground & odd)[:, None], col * CHECKER_DARK, col)
    shadow = np.zeros(d.shape[0], bool)
    if flags & FLAG_SHADOWS:
        sel = ground & (lam > 0)
        if sel.any():
            ts, _, _ = robot_hit(hp[sel], np.broadcast_to(light, hp[sel].shape), prims)
            shadow[np.flatnonzero(sel)] = np.isfinite(ts)
    lam = np.where(shadow, 0.0, lam)
    shade = AMBIENT + (1 - AMBIENT) * lam
    sky = ids == ID_SKY
    rgb = np.where(sky[:, None], col, col * shade[:, None])
    return dict(ids=ids, depth=t, rgb=rgb, shadow=shadow)


def to_uint8(rgb):
    return np.clip(np.floor(rgb * 255.0 + 0.5), 0, 255).astype(np.uint8)


def render(scene, k):
    """camera k: ids (H,W) int, depth (H,W), rgb (H,W,3) uint8, edge (H,W) bool"""
    W, H = scene["width"], scene["height"]
    c = trace(scene, k)
    edge = np.zeros(H * W, bool)
    for dx, dy in ((EDGE_EPS, 0), (-EDGE_EPS, 0), (0, EDGE_EPS), (0, -EDGE_EPS)):
        s = trace(scene, k, dx, dy)
        edge |= (s["ids"] != c["ids"]) | (s["shadow"] != c["shadow"])
    return c["ids"].reshape(H, W), c["depth"].reshape(H, W), to_uint8(c["rgb"]).reshape(H, W, 3), edge.reshape(H, W)


def standing_body_state(table_unused=None, root=(0.0, 0.0, 0.32), yaw=0.0, q=(0.0, 0.8, -1.5)):
    """(19,13) body rows of a Go2 standing with every leg at joint angles q (hip, thigh, calf), by the URDF's joint offsets: a pose for
    scenes that need a whole robot without an engine"""
    rows = np.zeros((19, 13))
    cz, sz = np.cos(yaw / 2), np.sin(yaw / 2)
    qb = np.array([0.0, 0.0, sz, cz]); Rb = quat_matrix(qb); root = np.asarray(root, np.float64)

    def qmul(a, b):
        return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                         a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    for b, off in enumerate(((0, 0, 0), (0.285, 0, 0.01), (0.293, 0, -0.06))):
        rows[b, :3] = root + Rb @ np.array(off, np.float64); rows[b, 3:7] = qb
    for leg, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        qh = np.array([np.sin(q[0] / 2), 0, 0, np.cos(q[0] / 2)])
        qt = qmul(qh, np.array([0, np.sin(q[1] / 2), 0, np.cos(q[1] / 2)]))
        qc = qmul(qt, np.array([0, np.sin(q[2] / 2), 0, np.cos(q[2] / 2)]))
        p_hip = np.array([sx * 0.1934, sy * 0.0465, 0.0])
        p_thigh = p_hip + quat_matrix(qh) @ np.array([0, sy * 0.0955, 0.0])
        p_calf = p_thigh + quat_matrix(qt) @ np.array([0, 0, -0.213])
        p_foot = p_calf + quat_matrix(qc) @ np.array([0, 0, -0.213])
        for j, (p, ql) in enumerate(((p_hip, qh), (p_thigh, qt), (p_calf, qc), (p_foot, qc))):
            rows[3 + 4 * leg + j, :3] = root + Rb @ p; rows[3 + 4 * leg + j, 3:7] = qmul(qb, ql)
    return rows
