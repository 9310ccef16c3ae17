// qa_obst_surface.h -- what a depth ray sees of an env's three articulated obstacles (see-saw, jump bar, tyre), ONCE,
// for host and device: the depth ray-cast (qa_depth.hip, qa_tsc_depth_update_obstacles) routes every floor / ceiling lookup of its march
// through these functions, and the host twin tests/c_host/qa_obst_surface_host.cpp calls the same functions on plain arrays.
//
// An env's record is 3 x 12 floats, the layout qa_sim.hip stages for contact_query (qa_physics.h):
//     [QA_T_OBST_DESC row: x, y, cos yaw, sin yaw, half length, half width, pivot height h0, kind | q, q_dot, tan q, damping]
// Float 10 is unused by the physics; here it carries tan q (qa_os_record_float), so that a lookup inside the see-saw's footprint costs one
// multiply and not one tangent.
//
// The rendered surface at world (x, y):
//   * footprint test: contact_query's -- lx = c dx + s dy, ly = c dy - s dx, inside when |lx| <= half length and |ly| <= half width and
//     kind != 0; the last matching slot wins, as there;
//   * see-saw footprint: floor = max(0, h0 - lx tan q), the plank's top plane  lx sin q + (z - h0) cos q = 0  (contact_query's pgap at r = 0)
//     over the ground at 0; the height map's A-frame is ignored, as the physics ignores it; the ceiling is left as the map has it;
//   * bar / tyre footprint: floor = map floor + q, ceiling = map ceiling + q (whether a ceiling triangle exists is the map's business);
//   * elsewhere: the map.
// The plank is solid beneath its top plane down to the ground, like every floor of a height field.  Its underside, its end faces and the
// QA_SEESAW_SHELL rule are collision concepts and are not rendered.
#ifndef QA_OBST_SURFACE_H
#define QA_OBST_SURFACE_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QA_OS_FN __host__ __device__ __forceinline__
#else
#define QA_OS_FN static inline
#endif

#define QA_OS_SLOTS 3             /* QA_OBST_PER_ENV */
#define QA_OS_RECORD 12
#define QA_OS_KIND_SEESAW 1.0f    /* QA_OBST_SEESAW; every other non-zero kind is a vertically shifted map (QA_OBST_BAR, QA_OBST_TYRE) */
#define QA_OS_NONE 0
#define QA_OS_SEESAW 1
#define QA_OS_SHIFT 2
#define QA_OS_BOX_PAD 1e-3f       /* m: the boxes of qa_os_box are grown by this much (rounding of the footprint test and of the march's cell lookup is ~1e-6 m) */

// float j of slot k's record from one env's QA_T_OBST_DESC (3,8) and QA_T_OBST_STATE (3,4) rows
QA_OS_FN float qa_os_record_float(const float *desc, const float *state, int k, int j) {
    if (j < 8) return desc[8 * k + j];
    if (j == 10) return tanf(state[4 * k]);
    return state[4 * k + (j - 8)];
}

typedef struct qa_os_cover {
    int mode;          // QA_OS_NONE / QA_OS_SEESAW / QA_OS_SHIFT
    float lx;          // along the obstacle's x axis, from its origin
    float h0, q, tq;   // pivot height, joint position, tan q of the covering slot
} qa_os_cover;

// which record covers (x, y)
QA_OS_FN qa_os_cover qa_os_classify(const float *rec, float x, float y) {
    qa_os_cover c; c.mode = QA_OS_NONE; c.lx = 0.f; c.h0 = 0.f; c.q = 0.f; c.tq = 0.f;
    for (int k = 0; k < QA_OS_SLOTS; ++k) {
        const float *d = rec + QA_OS_RECORD * k;
        const float kind = d[7];
        const float dx = x - d[0], dy = y - d[1];
        const float lx = d[2] * dx + d[3] * dy, ly = d[2] * dy - d[3] * dx;
        if (kind != 0.f && fabsf(lx) <= d[4] && fabsf(ly) <= d[5]) {
            c.mode = kind == QA_OS_KIND_SEESAW ? QA_OS_SEESAW : QA_OS_SHIFT; c.lx = lx; c.h0 = d[6]; c.q = d[8]; c.tq = d[10];
        }
    }
    return c;
}

QA_OS_FN float qa_os_floor(const qa_os_cover *c, float map_floor) {
    if (c->mode == QA_OS_SEESAW) return fmaxf(0.f, c->h0 - c->lx * c->tq);
    return c->mode == QA_OS_SHIFT ? map_floor + c->q : map_floor;
}

QA_OS_FN float qa_os_ceiling(const qa_os_cover *c, float map_ceiling) {
    return c->mode == QA_OS_SHIFT ? map_ceiling + c->q : map_ceiling;
}

// world-space axis-aligned box [x lo, x hi, y lo, y hi] of slot k's footprint, grown by QA_OS_BOX_PAD; an empty box (lo > hi) for kind 0.
// The ray-cast never skips a coarse block that overlaps one of them: the coarse maps bound the static map only.
QA_OS_FN void qa_os_box(const float *desc, int k, float box[4]) {
    const float *d = desc + 8 * k;
    if (d[7] == 0.f) { box[0] = box[2] = 3e38f; box[1] = box[3] = -3e38f; return; }       // (beyond the +-1e30 the ray-cast's outermost blocks extend to)
    const float ex = fabsf(d[2]) * d[4] + fabsf(d[3]) * d[5] + QA_OS_BOX_PAD, ey = fabsf(d[3]) * d[4] + fabsf(d[2]) * d[5] + QA_OS_BOX_PAD;
    box[0] = d[0] - ex; box[1] = d[0] + ex; box[2] = d[1] - ey; box[3] = d[1] + ey;
}

// does the ray (ox, oy) + t (dx, dy), 0 <= t <= t_max, pass over one of the boxes?  idx / idy: 1 / dx, 1 / dy, or 0 where the component is 0.
// A ray that passes over none takes no sample inside a footprint: its march is the static map's.
QA_OS_FN bool qa_os_ray_meets_boxes(const float *boxes /* 3 x 4 */, float ox, float oy, float dx, float dy, float idx, float idy, float t_max) {
    bool hit = false;
    for (int k = 0; k < QA_OS_SLOTS; ++k) {
        const float *b = boxes + 4 * k;
        bool ok = b[0] <= b[1];                                         // an empty box is met by nothing
        float t0 = 0.f, t1 = t_max;
        if (dx != 0.f) { const float ta = (b[0] - ox) * idx, tb = (b[1] - ox) * idx; t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb)); }
        else ok = ok && ox >= b[0] && ox <= b[1];
        if (dy != 0.f) { const float ta = (b[2] - oy) * idy, tb = (b[3] - oy) * idy; t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb)); }
        else ok = ok && oy >= b[2] && oy <= b[3];
        hit = hit || (ok && t0 <= t1);
    }
    return hit;
}

QA_OS_FN bool qa_os_boxes_overlap(const float *boxes /* 3 x 4 */, float x_lo, float x_hi, float y_lo, float y_hi) {
    bool hit = false;
    for (int k = 0; k < QA_OS_SLOTS; ++k) {
        const float *b = boxes + 4 * k;
        hit = hit || (x_lo <= b[1] && x_hi >= b[0] && y_lo <= b[3] && y_hi >= b[2]);
    }
    return hit;
}

#endif
