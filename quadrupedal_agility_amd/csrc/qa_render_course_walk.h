// qa_render_course_walk.h -- one pixel of the course renderer (include/qa_render_course.h), once for host and device: qa_render_course.hip
// calls qa_rc_pixel from its kernel with the staged arrays in LDS, tests/c_host/qa_render_course_host.cpp calls it on plain arrays, and
// tests/render_course_ref.py is its float64 twin.
//
// The ground is the surface of qa_obst_surface.h.  The exact walk of qa_render.hip is kept: the ray is cut at every lattice line, and
// besides at the (up to) nine parameters of the env's three records -- where the ray's (x, y) enters and leaves a footprint rectangle (a
// slab test in the obstacle's frame) and where the see-saw's plank plane h0 - lx tan q meets 0.  An extra cut never hurts: it splits a piece
// in two that lie in one plane.  Between two cuts the covering slot is constant; it is classified at the piece's midpoint (qa_os_classify),
// and the floor there is one plane: the map's, the map's + q, the plank's top, or z = 0.
// The cut parameters are per-ray constants in NAMED members (qa_rc_cuts), and "the smallest one beyond ta" is taken with compares: an array
// indexed by a loop-carried slot would go to scratch.
#ifndef QA_RENDER_COURSE_WALK_H
#define QA_RENDER_COURSE_WALK_H

#include "../../include/qa_render_course.h"
#include "qa_obst_surface.h"
#include "qa_render_walk.h"

namespace {

constexpr float QA_RC_NONE = 3.0e38f;

// pixel (i, j) of a `width` x `height` image of the camera row cam[7] (eye, target, vertical fov): the ray's origin and unit direction
QA_RS_HD void qa_rc_pixel_ray(const float *cam, int width, int height, int i, int j, float *o, float *d) {
    o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
    float f[3] = {cam[3] - o[0], cam[4] - o[1], cam[5] - o[2]};
    const float ifl = 1.0f / sqrtf(qa_rs_dot(f, f));
    f[0] *= ifl; f[1] *= ifl; f[2] *= ifl;
    float r[3] = {f[1], -f[0], 0.f};                                          // f x (0, 0, 1)
    float rl = r[0] * r[0] + r[1] * r[1];
    if (rl < 1e-12f) { r[0] = 0.f; r[1] = f[2]; r[2] = -f[1]; rl = r[1] * r[1] + r[2] * r[2]; }   // straight up / down: f x (1, 0, 0)
    const float irl = 1.0f / sqrtf(rl);
    r[0] *= irl; r[1] *= irl; r[2] *= irl;
    const float u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};   // r x f
    const float tv = tanf(0.5f * cam[6]), th = tv * (float)width / (float)height;
    const float sx = (((float)j + 0.5f) / (float)width * 2.0f - 1.0f) * th;
    const float sy = (1.0f - ((float)i + 0.5f) / (float)height * 2.0f) * tv;
    d[0] = f[0] + sx * r[0] + sy * u[0]; d[1] = f[1] + sx * r[1] + sy * u[1]; d[2] = f[2] + sx * r[2] + sy * u[2];
    const float idl = 1.0f / sqrtf(qa_rs_dot(d, d));
    d[0] *= idl; d[1] *= idl; d[2] *= idl;
}

// One record against the ray's (x, y): the parameters at which it enters and leaves the footprint rectangle (QA_RC_NONE both when it does
// not, or the slot is empty) and the rectangle side crossed there (0: a side of constant lx, 1: of constant ly); for a see-saw also the
// parameter at which h0 - lx tan q changes sign.  A parameter <= 0 lies behind the eye and is never taken.
struct qa_rc_slab { float t_in, t_out, t_zero; int side_in, side_out; float dlx, dly; };
QA_RS_HD qa_rc_slab qa_rc_slot_slab(const float *r, const float *o, const float *d) {
    qa_rc_slab s; s.t_in = s.t_out = s.t_zero = QA_RC_NONE; s.side_in = s.side_out = 0; s.dlx = s.dly = 0.f;
    if (r[7] == 0.f) return s;
    const float ex = o[0] - r[0], ey = o[1] - r[1];
    const float lx0 = r[2] * ex + r[3] * ey, ly0 = r[2] * ey - r[3] * ex;
    s.dlx = r[2] * d[0] + r[3] * d[1]; s.dly = r[2] * d[1] - r[3] * d[0];
    float t0 = -QA_RC_NONE, t1 = QA_RC_NONE;
    bool ok = true;
    if (s.dlx != 0.f) {
        const float inv = 1.0f / s.dlx, a = (-r[4] - lx0) * inv, b = (r[4] - lx0) * inv;
        t0 = fminf(a, b); t1 = fmaxf(a, b);
    } else ok = fabsf(lx0) <= r[4];
    if (s.dly != 0.f) {
        const float inv = 1.0f / s.dly, a = (-r[5] - ly0) * inv, b = (r[5] - ly0) * inv;
        const float n = fminf(a, b), f = fmaxf(a, b);
        if (n > t0) { t0 = n; s.side_in = 1; }
        if (f < t1) { t1 = f; s.side_out = 1; }
    } else ok = ok && fabsf(ly0) <= r[5];
    if (ok && t0 < t1) { s.t_in = t0; s.t_out = t1; }
    if (r[7] == QA_OS_KIND_SEESAW && r[10] != 0.f && s.dlx != 0.f) s.t_zero = (r[6] / r[10] - lx0) / s.dlx;
    return s;
}

struct qa_rc_cuts { float in0, out0, zero0, in1, out1, zero1, in2, out2, zero2; };

QA_RS_HD float qa_rc_nearer(float best, float v, float ta) { return (v > ta && v < best) ? v : best; }
// the smallest cut beyond ta that is nearer than tb
QA_RS_HD float qa_rc_next_cut(const qa_rc_cuts &c, float ta, float tb) {
    tb = qa_rc_nearer(tb, c.in0, ta); tb = qa_rc_nearer(tb, c.out0, ta); tb = qa_rc_nearer(tb, c.zero0, ta);
    tb = qa_rc_nearer(tb, c.in1, ta); tb = qa_rc_nearer(tb, c.out1, ta); tb = qa_rc_nearer(tb, c.zero1, ta);
    tb = qa_rc_nearer(tb, c.in2, ta); tb = qa_rc_nearer(tb, c.out2, ta); tb = qa_rc_nearer(tb, c.zero2, ta);
    return tb;
}
QA_RS_HD bool qa_rc_is_footprint_cut(const qa_rc_cuts &c, float t) {
    return t == c.in0 || t == c.out0 || t == c.in1 || t == c.out1 || t == c.in2 || t == c.out2;
}

// the horizontal unit normal of the rectangle side the ray crosses at the footprint cut `t`, turned against the ray.  Taken once per face
// hit, so the slabs are computed again here; the cut is recognised as the nearest of the six parameters.
QA_RS_HD void qa_rc_face_normal(const float *rec, const float *o, const float *d, float t, float *n) {
    float best = QA_RC_NONE;
    n[0] = 0.f; n[1] = 0.f; n[2] = 0.f;
    for (int k = 0; k < QA_OS_SLOTS; ++k) {
        const float *r = rec + QA_OS_RECORD * k;
        const qa_rc_slab s = qa_rc_slot_slab(r, o, d);
        for (int w = 0; w < 2; ++w) {
            const float tc = w ? s.t_out : s.t_in, dist = fabsf(tc - t);
            if (tc < QA_RC_NONE && dist < best) {
                best = dist;
                const int side = w ? s.side_out : s.side_in;
                const float sg = (side ? s.dly : s.dlx) > 0.f ? -1.f : 1.f;
                n[0] = sg * (side ? -r[3] : r[2]); n[1] = sg * (side ? r[2] : r[3]);
            }
        }
    }
}

// the see-saw slot whose footprint holds (x, y): qa_os_classify's test and order (the last matching slot wins), restricted to see-saws
QA_RS_HD int qa_rc_seesaw_slot(const float *rec, float x, float y) {
    int slot = 0;
    for (int k = 0; k < QA_OS_SLOTS; ++k) {
        const float *r = rec + QA_OS_RECORD * k;
        const float dx = x - r[0], dy = y - r[1];
        const float lx = r[2] * dx + r[3] * dy, ly = r[2] * dy - r[3] * dx;
        if (r[7] == QA_OS_KIND_SEESAW && fabsf(lx) <= r[4] && fabsf(ly) <= r[5]) slot = k;
    }
    return slot;
}

// The ground walk on (0, tend): the first crossing of the drawn floor from above, of an existing ceiling triangle either way, or a vertical
// face at a footprint cut.  Returns QA_RENDER_ID_SKY when there is none; else the id, with *t_out and n set.  rec: the env's 36 record floats.
QA_RS_HD int qa_rc_ground(const float *rec, const int16_t *__restrict__ hm, const int16_t *__restrict__ cm, int rows, int cols, float border, float inv_hs,
                          float vs, const float *o, const float *d, float tend, float *t_out, float *n) {
    qa_rc_cuts cuts;
    { const qa_rc_slab s = qa_rc_slot_slab(rec, o, d); cuts.in0 = s.t_in; cuts.out0 = s.t_out; cuts.zero0 = s.t_zero; }
    { const qa_rc_slab s = qa_rc_slot_slab(rec + QA_OS_RECORD, o, d); cuts.in1 = s.t_in; cuts.out1 = s.t_out; cuts.zero1 = s.t_zero; }
    { const qa_rc_slab s = qa_rc_slot_slab(rec + 2 * QA_OS_RECORD, o, d); cuts.in2 = s.t_in; cuts.out2 = s.t_out; cuts.zero2 = s.t_zero; }
    const float fx0 = (o[0] + border) * inv_hs, fy0 = (o[1] + border) * inv_hs;
    const float dfx = d[0] * inv_hs, dfy = d[1] * inv_hs;
    Line lx = line_init(fx0, dfx), ly = line_init(fy0, dfy), ld = line_init(fx0 - fy0, dfx - dfy);
    float tx = line_t(lx), ty = line_t(ly), td = line_t(ld);
    float ta = 0.f, g_prev = -1.f;                                           // (a ray sees no face at its start)
    int id = QA_RENDER_ID_SKY;
    while (ta < tend) {
        const float tb = qa_rc_next_cut(cuts, ta, fminf(fminf(tx, ty), fminf(td, tend)));
        const float tm = 0.5f * (ta + tb);
        const float fxm = fx0 + tm * dfx, fym = fy0 + tm * dfy;
        const float fxa = fx0 + ta * dfx, fya = fy0 + ta * dfy, fxb = fx0 + tb * dfx, fyb = fy0 + tb * dfy;
        const float za = o[2] + ta * d[2], zb = o[2] + tb * d[2];
        const float xm = o[0] + tm * d[0], ym = o[1] + tm * d[1];
        const qa_os_cover cv = qa_os_classify(rec, xm, ym);
        const Piece pf = piece_at(hm, rows, cols, vs, fxm, fym);
        float fa, fb;
        const bool plank = cv.mode == QA_OS_SEESAW && qa_os_floor(&cv, 0.f) > 0.f;
        if (plank) {                                                        // the plank's top plane, taken at the piece's two ends
            const float *r = rec + QA_OS_RECORD * qa_rc_seesaw_slot(rec, xm, ym);
            const float lxa = r[2] * (o[0] + ta * d[0] - r[0]) + r[3] * (o[1] + ta * d[1] - r[1]);
            const float lxb = r[2] * (o[0] + tb * d[0] - r[0]) + r[3] * (o[1] + tb * d[1] - r[1]);
            fa = cv.h0 - lxa * cv.tq; fb = cv.h0 - lxb * cv.tq;
        } else if (cv.mode == QA_OS_SEESAW) {
            fa = 0.f; fb = 0.f;
        } else {
            fa = qa_os_floor(&cv, piece_height(pf, fxa, fya)); fb = qa_os_floor(&cv, piece_height(pf, fxb, fyb));
        }
        const float ga = za - fa, gb = zb - fb;
        if (g_prev >= 0.f && ga < 0.f && qa_rc_is_footprint_cut(cuts, ta)) {  // the floor jumps up at a footprint's edge: its vertical face
            qa_rc_face_normal(rec, o, d, ta, n);
            *t_out = ta;
            return QA_RENDER_ID_OBSTACLE_SIDE;
        }
        float th_ = QA_RC_NONE;
        if (ga >= 0.f && gb < 0.f) {                                         // from above, inside this piece: the plane's crossing
            th_ = ta + (tb - ta) * (ga / (ga - gb));
            if (plank) {
                const float *r = rec + QA_OS_RECORD * qa_rc_seesaw_slot(rec, xm, ym);
                const float il = 1.0f / sqrtf(cv.tq * cv.tq + 1.f);
                n[0] = r[2] * cv.tq * il; n[1] = r[3] * cv.tq * il; n[2] = il;
                id = QA_RENDER_ID_OBSTACLE;
            } else if (cv.mode == QA_OS_SEESAW) {
                n[0] = 0.f; n[1] = 0.f; n[2] = 1.f;
                id = QA_RENDER_ID_GROUND;
            } else {
                piece_normal(pf, fxm, fym, rows, cols, inv_hs, n);
                id = cv.mode == QA_OS_SHIFT ? QA_RENDER_ID_OBSTACLE : QA_RENDER_ID_GROUND;
            }
        }
        if (cm) {
            const Piece pc = piece_at(cm, rows, cols, vs, fxm, fym);
            if (pc.exists) {
                const float ha = za - qa_os_ceiling(&cv, piece_height(pc, fxa, fya)), hb = zb - qa_os_ceiling(&cv, piece_height(pc, fxb, fyb));
                if ((ha < 0.f) != (hb < 0.f)) {                              // a thin shell: from below or from above
                    const float tc = ta + (tb - ta) * (ha / (ha - hb));
                    if (tc < th_) {
                        th_ = tc; id = QA_RENDER_ID_CEILING;
                        piece_normal(pc, fxm, fym, rows, cols, inv_hs, n);
                        if (ha < 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }     // seen from below: the underside
                    }
                }
            }
        }
        if (th_ < 1.0e38f) { *t_out = fminf(th_, tend); return id; }
        if (tx <= tb) { lx.m += lx.step; tx = line_t(lx); }
        if (ty <= tb) { ly.m += ly.step; ty = line_t(ly); }
        if (td <= tb) { ld.m += ld.step; td = line_t(ld); }
        g_prev = gb;
        ta = tb;
    }
    return QA_RENDER_ID_SKY;
}

// One pixel's ray (table / palette: the caller's side's copies, see stage_prim): the nearest of the robot (prims: 23 x PRIM_FLOATS in the world frame), the goals (num_goals centres; 0 for none) and the
// ground, shaded.  Writes the colour as floats in [0, 1]; returns the id, *t_out the distance (`far` on a miss).
QA_RS_HD int qa_rc_pixel(const qa_rs_prim *table, const float *palette, const float *prims, const float *rec, const float *goals, int num_goals, float goal_radius, int cur_goal, int reached,
                         const int16_t *__restrict__ hm, const int16_t *__restrict__ cm, int rows, int cols, float border, float inv_hs, float vs,
                         float far, const float *light, int flags, const float *o, const float *d, float *t_out, float *col) {
    float t = far, n[3] = {0.f, 0.f, 1.f};
    int id = QA_RENDER_ID_SKY, cls = QA_RS_CLS_SKY;
    const int pi = robot_hit(table, prims, o, d, far, &t, n);
    if (pi >= 0) { id = table[pi].body; cls = table[pi].cls; }
    for (int g = 0; g < num_goals; ++g) {
        float tg, ng[3];
        if (qa_rs_ray_sphere(o, d, goals + 3 * g, goal_radius, &tg, ng) && tg < t) {
            t = tg; n[0] = ng[0]; n[1] = ng[1]; n[2] = ng[2];
            id = g != cur_goal ? QA_RENDER_ID_GOAL : reached ? QA_RENDER_ID_GOAL_REACHED : QA_RENDER_ID_GOAL_CURRENT;
        }
    }
    {
        float tg, ng[3];
        const int gid = qa_rc_ground(rec, hm, cm, rows, cols, border, inv_hs, vs, o, d, t, &tg, ng);   // nothing behind the nearer hit (or `far`) is looked at
        if (gid != QA_RENDER_ID_SKY) { id = gid; t = tg; n[0] = ng[0]; n[1] = ng[1]; n[2] = ng[2]; }
    }
    if (id == QA_RENDER_ID_GROUND) cls = QA_RS_CLS_GROUND;
    if (id == QA_RENDER_ID_CEILING) cls = QA_RS_CLS_CEILING;
    col[0] = palette[3 * cls]; col[1] = palette[3 * cls + 1]; col[2] = palette[3 * cls + 2];
    if (id == QA_RENDER_ID_OBSTACLE || id == QA_RENDER_ID_OBSTACLE_SIDE) { col[0] = QA_RENDER_COL_OBSTACLE_R; col[1] = QA_RENDER_COL_OBSTACLE_G; col[2] = QA_RENDER_COL_OBSTACLE_B; }
    if (id == QA_RENDER_ID_GOAL) { col[0] = QA_RENDER_COL_GOAL_R; col[1] = QA_RENDER_COL_GOAL_G; col[2] = QA_RENDER_COL_GOAL_B; }
    if (id == QA_RENDER_ID_GOAL_CURRENT) { col[0] = QA_RENDER_COL_GOAL_CURRENT_R; col[1] = QA_RENDER_COL_GOAL_CURRENT_G; col[2] = QA_RENDER_COL_GOAL_CURRENT_B; }
    if (id == QA_RENDER_ID_GOAL_REACHED) { col[0] = QA_RENDER_COL_GOAL_REACHED_R; col[1] = QA_RENDER_COL_GOAL_REACHED_G; col[2] = QA_RENDER_COL_GOAL_REACHED_B; }
    if (id != QA_RENDER_ID_SKY) {
        const float hp[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        float lam = fmaxf(qa_rs_dot(n, light), 0.f);
        if (id == QA_RENDER_ID_GROUND && (flags & QA_RENDER_CHECKER) &&
            (((int)floorf(hp[0] * (1.0f / QA_RENDER_CHECKER_SIZE)) + (int)floorf(hp[1] * (1.0f / QA_RENDER_CHECKER_SIZE))) & 1)) {
            col[0] *= QA_RENDER_CHECKER_DARK; col[1] *= QA_RENDER_CHECKER_DARK; col[2] *= QA_RENDER_CHECKER_DARK;
        }
        if ((id == QA_RENDER_ID_GROUND || id == QA_RENDER_ID_OBSTACLE) && (flags & QA_RENDER_SHADOWS) && lam > 0.f) {
            float ts, ns[3];
            if (robot_hit(table, prims, hp, light, 3.0e38f, &ts, ns) >= 0) lam = 0.f;
        }
        const float shade = QA_RENDER_AMBIENT + (1.0f - QA_RENDER_AMBIENT) * lam;
        col[0] *= shade; col[1] *= shade; col[2] *= shade;
    }
    *t_out = t;
    return id;
}

}  // namespace

#endif
