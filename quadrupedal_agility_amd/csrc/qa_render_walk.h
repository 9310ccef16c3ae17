// qa_render_walk.h -- what the frame renderer's two kernels share (qa_render.hip, qa_render_course.hip): the launch arguments, the robot's
// primitives in the world frame, the nearest robot hit, and the pieces and lattice lines of the height field's exact walk.  Once for host
// and device like qa_render_shapes.h: tests/c_host/qa_render_course_host.cpp compiles it with the host compiler.
#ifndef QA_RENDER_WALK_H
#define QA_RENDER_WALK_H

#include <math.h>
#include <stdint.h>

#include "../../include/qa_render.h"
#include "qa_render_shapes.h"

namespace {     // (a header with an unnamed namespace: every unit that includes it gets its own copy, and the kernels' symbols keep their names)

// trunk, hip, thigh, calf, foot, ground, ceiling, sky
const float PALETTE[QA_RS_NUM_CLASSES][3] = {{0.80f, 0.80f, 0.82f}, {0.25f, 0.25f, 0.28f}, {0.90f, 0.55f, 0.15f}, {0.20f, 0.45f, 0.85f},
                                             {0.85f, 0.15f, 0.15f}, {0.55f, 0.60f, 0.50f}, {0.60f, 0.45f, 0.35f}, {0.55f, 0.75f, 0.95f}};
#if defined(__HIPCC__)
__constant__ float PALETTE_DEV[QA_RS_NUM_CLASSES][3] = {{0.80f, 0.80f, 0.82f}, {0.25f, 0.25f, 0.28f}, {0.90f, 0.55f, 0.15f}, {0.20f, 0.45f, 0.85f},
                                                        {0.85f, 0.15f, 0.15f}, {0.55f, 0.60f, 0.50f}, {0.60f, 0.45f, 0.35f}, {0.55f, 0.75f, 0.95f}};
#endif

struct RenderArgs {
    qa_render_cfg c;
    qa_render_io io;
    float light[3];         // unit
    float inv_hs;
    int tiles_x;
};

// a primitive in the world frame: [0..2] centre / capsule end a, [3..5] capsule end b / box half sizes, [6..14] box axes (row-major body -> world),
// [15] radius, [16..19] bounding sphere (centre, radius)
constexpr int PRIM_FLOATS = 20;

QA_RS_HD int qa_rw_mini(int a, int b) { return a < b ? a : b; }
QA_RS_HD int qa_rw_maxi(int a, int b) { return a > b ? a : b; }

// `table`: the primitive table of the side that runs this (QA_RS_TABLE_DEV in a kernel, QA_RS_TABLE on the host).  A parameter, not a choice
// made in here: a static __constant__ that a __host__ __device__ function names is given external linkage, and the kernels would reach it
// through the GOT.
QA_RS_HD void stage_prim(const qa_rs_prim *table, const float *__restrict__ rows, int i, float *w) {
    const qa_rs_prim &p = table[i];
    const float *r = rows + 13 * p.body;
    float R[9];
    qa_rs_quat_matrix(r + 3, R);
    for (int k = 0; k < 3; ++k) w[k] = r[k] + R[3 * k] * p.a[0] + R[3 * k + 1] * p.a[1] + R[3 * k + 2] * p.a[2];
    for (int k = 0; k < 9; ++k) w[6 + k] = R[k];
    w[15] = p.r;
    if (p.kind == QA_RS_CAPSULE) {
        for (int k = 0; k < 3; ++k) w[3 + k] = r[k] + R[3 * k] * p.b[0] + R[3 * k + 1] * p.b[1] + R[3 * k + 2] * p.b[2];
        const float h[3] = {0.5f * (w[3] - w[0]), 0.5f * (w[4] - w[1]), 0.5f * (w[5] - w[2])};
        for (int k = 0; k < 3; ++k) w[16 + k] = w[k] + h[k];
        w[19] = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]) + p.r;
    } else {
        for (int k = 0; k < 3; ++k) { w[3 + k] = p.b[k]; w[16 + k] = w[k]; }
        w[19] = p.kind == QA_RS_BOX ? sqrtf(p.b[0] * p.b[0] + p.b[1] * p.b[1] + p.b[2] * p.b[2]) : p.r;
    }
    w[19] *= 1.0001f;       // the exact test decides; the bound only has to be no smaller than the primitive
}

// nearest robot hit on (0, tmax): returns the primitive's index or -1
QA_RS_HD int robot_hit(const qa_rs_prim *table, const float *s_prim, const float *o, const float *d, float tmax, float *t_out, float *n_out) {
    int best = -1;
    float tb = tmax;
    for (int i = 0; i < QA_RS_NUM_PRIMS; ++i) {
        const float *w = s_prim + i * PRIM_FLOATS;
        const float oc[3] = {o[0] - w[16], o[1] - w[17], o[2] - w[18]};
        const float b = qa_rs_dot(oc, d);
        const float p[3] = {oc[0] - b * d[0], oc[1] - b * d[1], oc[2] - b * d[2]};
        const float rr = w[19] * w[19];
        if (qa_rs_dot(p, p) > rr) continue;                                  // the line misses the bounding sphere
        if (b > 0.f && qa_rs_dot(oc, oc) > rr) continue;                      // the sphere lies behind the origin
        float t, n[3];
        const int kind = table[i].kind;
        int hit;
        if (kind == QA_RS_SPHERE) hit = qa_rs_ray_sphere(o, d, w, w[15], &t, n);
        else if (kind == QA_RS_CAPSULE) hit = qa_rs_ray_capsule(o, d, w, w + 3, w[15], &t, n);
        else hit = qa_rs_ray_box(o, d, w, w + 6, w + 3, &t, n);
        if (hit && t < tb) { tb = t; best = i; n_out[0] = n[0]; n_out[1] = n[1]; n_out[2] = n[2]; }
    }
    *t_out = tb;
    return best;
}

// the plane of the map's piece that holds lattice position (fxm, fym): its value at (fx, fy) (lookup clamped like cell_of), whether it
// exists (a ceiling triangle with a QA_NO_CEILING corner does not) and its gradient per metre
struct Piece { int ix, iy; bool lower, exists; float h00, hm, h11; };
QA_RS_HD Piece piece_at(const int16_t *__restrict__ m, int rows, int cols, float vs, float fxm, float fym) {
    Piece p;
    p.ix = qa_rw_mini(qa_rw_maxi((int)floorf(fxm), 0), rows - 2); p.iy = qa_rw_mini(qa_rw_maxi((int)floorf(fym), 0), cols - 2);
    const float u = fminf(fmaxf(fxm - (float)p.ix, 0.f), 1.f), v = fminf(fmaxf(fym - (float)p.iy, 0.f), 1.f);
    p.lower = u >= v;
    const int16_t *g = m + (int64_t)p.ix * cols + p.iy;
    const int s00 = g[0], s11 = g[cols + 1], sm = p.lower ? g[cols] : g[1];
    p.exists = s00 != QA_NO_CEILING && s11 != QA_NO_CEILING && sm != QA_NO_CEILING;
    p.h00 = vs * (float)s00; p.h11 = vs * (float)s11; p.hm = vs * (float)sm;
    return p;
}
QA_RS_HD float piece_height(const Piece &p, float fx, float fy) {
    const float u = fminf(fmaxf(fx - (float)p.ix, 0.f), 1.f), v = fminf(fmaxf(fy - (float)p.iy, 0.f), 1.f);
    const float a = p.lower ? u : v, b = p.lower ? v : u;
    return p.h00 + a * (p.hm - p.h00) + b * (p.h11 - p.hm);
}
QA_RS_HD void piece_normal(const Piece &p, float fxm, float fym, int rows, int cols, float inv_hs, float *n) {
    // lower: dH/du = hm - h00, dH/dv = h11 - hm; upper: dH/du = h11 - hm, dH/dv = hm - h00; outside the map the clamped direction is flat
    float gu = p.lower ? p.hm - p.h00 : p.h11 - p.hm, gv = p.lower ? p.h11 - p.hm : p.hm - p.h00;
    if (fxm < 0.f || fxm > (float)(rows - 1)) gu = 0.f;
    if (fym < 0.f || fym > (float)(cols - 1)) gv = 0.f;
    const float nx = -gu * inv_hs, ny = -gv * inv_hs, il = 1.0f / sqrtf(nx * nx + ny * ny + 1.f);
    n[0] = nx * il; n[1] = ny * il; n[2] = il;
}

// first lattice line after the start for one family: position f0, speed df per unit t; `m` is the next integer the ray meets
struct Line { float f0, inv; int m, step; };
QA_RS_HD Line line_init(float f0, float df) {
    Line l; l.f0 = f0;
    if (df > 0.f) { l.m = (int)floorf(f0) + 1; l.step = 1; l.inv = 1.0f / df; }
    else if (df < 0.f) { l.m = (int)ceilf(f0) - 1; l.step = -1; l.inv = 1.0f / df; }
    else { l.m = 0; l.step = 0; l.inv = 0.f; }
    return l;
}
QA_RS_HD float line_t(const Line &l) { return l.step ? ((float)l.m - l.f0) * l.inv : 3.0e38f; }

}  // namespace

#endif
