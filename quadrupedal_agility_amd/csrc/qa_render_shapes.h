/* qa_render_shapes.h -- the primitives the frame renderer (qa_render.hip, include/qa_render.h) draws for the Go2's 19 bodies, and the
 * ray-primitive intersections, once for host and device (the pattern of qa_obst_surface.h / qa_selfcol.h: plain floats, no HIP type).
 * tests/c_host/qa_render_shapes_host.cpp compiles this header with the host compiler; tests/render_ref.py is its float64 twin.
 *
 * The table restates the <collision> elements of the Go2 URDF (resources/robots/go2/urdf/go2.urdf of the reference) as numbers, written by
 * hand the way qa_go2_model.h restates the inertias; each primitive is given in the frame of the body whose QA_T_RIGID_BODY_STATE row poses it
 * (bodies in _capi.BODY_NAMES order: base, Head_upper, Head_lower, then hip / thigh / calf / foot of FL, FR, RL, RR):
 *   base        box 0.3762 x 0.0935 x 0.114 at the origin
 *   Head_upper  the URDF has a cylinder r 0.05, length 0.09 along z: drawn as its bounding BOX 0.1 x 0.1 x 0.09
 *   Head_lower  sphere r 0.047
 *   hip         cylinder r 0.046, length 0.04 along y at y = +-0.08 (+ left legs, - right legs): drawn as a CAPSULE on the cylinder's axis
 *               segment, i.e. with round ends of r 0.046 beyond the flat caps
 *   thigh       box 0.11 x 0.0245 x 0.034 pitched by 90 deg at z = -0.1065: in the thigh frame half sizes (0.017, 0.01225, 0.055)
 *   calf        two capsules: the calf link's cylinder (r 0.013, length 0.12, pitch -0.2 at (0.01, 0, -0.06); FL's 0.012 / -0.21 / 0.008 are
 *               not distinguished), and from its lower end to the foot's centre with calflower's r 0.011 (the taper of calflower1 is ignored)
 *   foot        sphere r 0.022 at (-0.002, 0, 0)
 * Every box is axis-aligned in its body's frame, so a box carries no rotation of its own.
 *
 * Rays: origin o, UNIT direction d.  Each function returns 1 and writes the hit parameter t (> 0, a distance) and the outward unit normal,
 * or returns 0.  A ray that starts inside a primitive (or on its surface) reports no hit.
 */
#ifndef QA_RENDER_SHAPES_H
#define QA_RENDER_SHAPES_H

#include <math.h>

#if defined(__HIPCC__)
#define QA_RS_HD __host__ __device__ __forceinline__
#else
#define QA_RS_HD static inline
#endif

#define QA_RS_SPHERE 0      /* a = centre, r */
#define QA_RS_CAPSULE 1     /* a, b = the segment's ends, r */
#define QA_RS_BOX 2         /* a = centre, b = half sizes along the body's axes */

/* colour classes (qa_render.hip's palette) */
#define QA_RS_CLS_TRUNK 0
#define QA_RS_CLS_HIP 1
#define QA_RS_CLS_THIGH 2
#define QA_RS_CLS_CALF 3
#define QA_RS_CLS_FOOT 4
#define QA_RS_CLS_GROUND 5
#define QA_RS_CLS_CEILING 6
#define QA_RS_CLS_SKY 7
#define QA_RS_NUM_CLASSES 8

#define QA_RS_NUM_BODIES 19
#define QA_RS_NUM_PRIMS 23

typedef struct qa_rs_prim {
    int kind, body, cls;
    float a[3], b[3], r;
} qa_rs_prim;

/* one leg: `b0` = the hip's body index, `sy` = +1 (left) / -1 (right) */
#define QA_RS_LEG(b0, sy)                                                                                                          \
    {QA_RS_CAPSULE, (b0), QA_RS_CLS_HIP, {0.f, (sy) * 0.08f - 0.02f, 0.f}, {0.f, (sy) * 0.08f + 0.02f, 0.f}, 0.046f},               \
    {QA_RS_BOX, (b0) + 1, QA_RS_CLS_THIGH, {0.f, 0.f, -0.1065f}, {0.017f, 0.01225f, 0.055f}, 0.f},                                  \
    {QA_RS_CAPSULE, (b0) + 2, QA_RS_CLS_CALF, {-0.0019201f, 0.f, -0.001196f}, {0.0219201f, 0.f, -0.118804f}, 0.013f},               \
    {QA_RS_CAPSULE, (b0) + 2, QA_RS_CLS_CALF, {0.0219201f, 0.f, -0.118804f}, {-0.002f, 0.f, -0.213f}, 0.011f},                      \
    {QA_RS_SPHERE, (b0) + 3, QA_RS_CLS_FOOT, {-0.002f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.022f}

#define QA_RS_TABLE_INIT {                                                                                                         \
    {QA_RS_BOX, 0, QA_RS_CLS_TRUNK, {0.f, 0.f, 0.f}, {0.1881f, 0.04675f, 0.057f}, 0.f},                                             \
    {QA_RS_BOX, 1, QA_RS_CLS_TRUNK, {0.f, 0.f, 0.f}, {0.05f, 0.05f, 0.045f}, 0.f},                                                  \
    {QA_RS_SPHERE, 2, QA_RS_CLS_TRUNK, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0.047f},                                                   \
    QA_RS_LEG(3, 1.f), QA_RS_LEG(7, -1.f), QA_RS_LEG(11, 1.f), QA_RS_LEG(15, -1.f) }

static const qa_rs_prim QA_RS_TABLE[QA_RS_NUM_PRIMS] = QA_RS_TABLE_INIT;          /* the host's copy */
#if defined(__HIPCC__)
static __constant__ qa_rs_prim QA_RS_TABLE_DEV[QA_RS_NUM_PRIMS] = QA_RS_TABLE_INIT; /* the kernels' copy */
#endif

QA_RS_HD float qa_rs_dot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* Sphere (c, r).  The discriminant is taken as r^2 - |oc - (oc.d) d|^2 (the squared distance of the centre from the ray's line): it does not
 * cancel two squares of the distance to the sphere, which the textbook b^2 - c does for a far camera.  t counts in units of |d|. */
QA_RS_HD int qa_rs_ray_sphere(const float *o, const float *d, const float *c, float r, float *t, float *n) {
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const float idd = 1.0f / qa_rs_dot(d, d);            /* 1 up to the direction's own rounding: left at 1 that error would enter as (oc.d)^2 / r */
    const float b = qa_rs_dot(oc, d) * idd;
    const float p[3] = {oc[0] - b * d[0], oc[1] - b * d[1], oc[2] - b * d[2]};
    const float disc = (r * r - qa_rs_dot(p, p)) * idd;
    if (!(disc > 0.f) || qa_rs_dot(oc, oc) <= r * r) return 0;
    const float s = -b - sqrtf(disc);
    if (!(s > 0.f)) return 0;
    const float ir = 1.0f / r;
    *t = s;
    n[0] = (oc[0] + s * d[0]) * ir; n[1] = (oc[1] + s * d[1]) * ir; n[2] = (oc[2] + s * d[2]) * ir;
    return 1;
}

/* Capsule (segment a-b, r) = the union of the two end spheres and the finite cylinder between them.  A ray from outside enters the union
 * where it first enters one of the three, and it cannot enter the finite cylinder through a flat end without having entered that end's
 * sphere before: the hit is the smallest of {sphere a, sphere b, the infinite cylinder's side where it lies between the ends}.  A ray along
 * the axis has no side hit (the quadratic's leading term vanishes) and is left to the spheres. */
QA_RS_HD int qa_rs_ray_capsule(const float *o, const float *d, const float *a, const float *b, float r, float *t, float *n) {
    const float ba[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float oa[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    const float len2 = qa_rs_dot(ba, ba), il = 1.0f / sqrtf(len2);
    const float u[3] = {ba[0] * il, ba[1] * il, ba[2] * il};
    const float du = qa_rs_dot(d, u), ou = qa_rs_dot(oa, u), len = len2 * il;
    /* the start's distance from the segment: inside -> no hit */
    const float sc = fminf(fmaxf(ou, 0.f), len);
    const float q[3] = {oa[0] - sc * u[0], oa[1] - sc * u[1], oa[2] - sc * u[2]};
    if (qa_rs_dot(q, q) <= r * r) return 0;
    float best = 3.0e38f, tn, nn[3];
    int hit = 0;
    /* side: components perpendicular to the axis */
    const float dp[3] = {d[0] - du * u[0], d[1] - du * u[1], d[2] - du * u[2]};
    const float op[3] = {oa[0] - ou * u[0], oa[1] - ou * u[1], oa[2] - ou * u[2]};
    const float A = qa_rs_dot(dp, dp);
    if (A > 1e-12f) {
        const float iA = 1.0f / A, m = qa_rs_dot(op, dp) * iA;            /* -m = the parameter of the closest approach to the axis */
        const float w[3] = {op[0] - m * dp[0], op[1] - m * dp[1], op[2] - m * dp[2]};
        const float disc = r * r - qa_rs_dot(w, w);
        if (disc > 0.f) {
            const float s = -m - sqrtf(disc * iA), y = ou + s * du;
            if (s > 0.f && y > 0.f && y < len) {
                const float ir = 1.0f / r;
                best = s; hit = 1;
                n[0] = (op[0] + s * dp[0]) * ir; n[1] = (op[1] + s * dp[1]) * ir; n[2] = (op[2] + s * dp[2]) * ir;
            }
        }
    }
    if (qa_rs_ray_sphere(o, d, a, r, &tn, nn) && tn < best) { best = tn; hit = 1; n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2]; }
    if (qa_rs_ray_sphere(o, d, b, r, &tn, nn) && tn < best) { best = tn; hit = 1; n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2]; }
    if (hit) *t = best;
    return hit;
}

/* Oriented box: centre c, axes = the COLUMNS of the row-major rotation R (body -> world), half sizes h.  Slab test in the body frame; a
 * direction component of exactly 0 takes no division: the ray is inside that slab for all t or for none. */
QA_RS_HD int qa_rs_ray_box(const float *o, const float *d, const float *c, const float *R, const float *h, float *t, float *n) {
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    float tmin = -3.0e38f, tmax = 3.0e38f, sgn = 0.f;
    int axis = 0;
    for (int i = 0; i < 3; ++i) {
        const float ol = R[i] * oc[0] + R[3 + i] * oc[1] + R[6 + i] * oc[2];
        const float dl = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
        if (dl == 0.f) {
            if (fabsf(ol) >= h[i]) return 0;
            continue;
        }
        const float inv = 1.0f / dl;
        const float t1 = (-h[i] - ol) * inv, t2 = (h[i] - ol) * inv;
        const float tn = fminf(t1, t2), tf = fmaxf(t1, t2);
        if (tn > tmin) { tmin = tn; axis = i; sgn = dl > 0.f ? -1.f : 1.f; }
        tmax = fminf(tmax, tf);
    }
    if (!(tmin < tmax) || !(tmin > 0.f)) return 0;
    *t = tmin;
    n[0] = sgn * R[axis]; n[1] = sgn * R[3 + axis]; n[2] = sgn * R[6 + axis];
    return 1;
}

/* row-major rotation (body -> world) of a unit quaternion (x, y, z, w) */
QA_RS_HD void qa_rs_quat_matrix(const float *q, float *R) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - z * w); R[2] = 2.f * (x * z + y * w);
    R[3] = 2.f * (x * y + z * w); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - x * w);
    R[6] = 2.f * (x * z - y * w); R[7] = 2.f * (y * z + x * w); R[8] = 1.f - 2.f * (x * x + y * y);
}

#endif
