// qa_selfcol.h -- the geometry of the calf-against-neighbouring-hip and calf-against-neighbouring-thigh self-collision classes
// (include/qa_sim_selfcol.h), ONCE, for host and device: phys_substep (qa_physics.h) calls these functions with base-frame points
// it holds in registers, and the host twins tests/c_host/qa_selfcol_host.cpp and qa_selfcol_thighs_host.cpp call the same functions on plain
// arrays.  Plain floats in, plain floats out.
//
// Shapes, base frame: the calf is the capsule of the calf-calf class (knee to foot centre, radius QA_CALF_RADIUS at the knee growing to
// QA_FOOT_RADIUS at the foot); the hip is the URDF's hip cylinder taken as a capsule -- segment (0, +-0.06, 0) .. (0, +-0.10, 0) in the hip
// link's frame (+ for left legs), radius 0.046 m.  It rides on the hip link: only joint 0 (about x, at the hip joint origin) moves it.
// The capsule's rounded ends reach 46 mm past the cylinder's flat faces: conservative by design (a calf is stopped early there, never late).
#ifndef QA_SELFCOL_H
#define QA_SELFCOL_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QA_SC_FN __host__ __device__ __forceinline__
#define QA_SC_UNROLL _Pragma("unroll")
#else
#define QA_SC_FN static inline
#define QA_SC_UNROLL
#endif

#ifndef QA_CALF_RADIUS
#define QA_CALF_RADIUS 0.013f
#define QA_FOOT_RADIUS 0.022f
#endif
#define QA_HIP_CAP_RADIUS 0.046f
#define QA_HIP_CAP_Y0 0.06f
#define QA_HIP_CAP_Y1 0.10f

typedef struct qa_sc_contact {
    float gap;        // surface distance (m): < 0 penetrating
    float s, t;       // parameters of the closest points on the calf (knee -> foot) and on the hip segment
    float n[3];       // unit normal from the hip's point to the calf's: the force on the calf is +n, on the hip -n
    float pc[3];      // closest point on the calf segment
    float ph[3];      // closest point on the hip segment
} qa_sc_contact;

// the hip capsule's segment from the hip joint origin, cos / sin of joint 0 and the leg's side (+1 left, -1 right): org + side y Rx(q0) e_y
QA_SC_FN void qa_sc_hip_segment(const float org[3], float c1, float s1, float side, float h0[3], float h1[3]) {
    const float y0 = side * QA_HIP_CAP_Y0, y1 = side * QA_HIP_CAP_Y1;
    h0[0] = org[0]; h0[1] = org[1] + y0 * c1; h0[2] = org[2] + y0 * s1;
    h1[0] = org[0]; h1[1] = org[1] + y1 * c1; h1[2] = org[2] + y1 * s1;
}

QA_SC_FN float qa_sc_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// closest points of segments A0 + s (A1 - A0), B0 + t (B1 - B0): the expressions of segment_closest (qa_physics.h; Ericson 5.1.9) on plain arrays
QA_SC_FN void qa_sc_segment_closest(const float A0[3], const float A1[3], const float B0[3], const float B1[3], float *s_, float *t_) {
    const float d1[3] = {A1[0] - A0[0], A1[1] - A0[1], A1[2] - A0[2]}, d2[3] = {B1[0] - B0[0], B1[1] - B0[1], B1[2] - B0[2]};
    const float r[3] = {A0[0] - B0[0], A0[1] - B0[1], A0[2] - B0[2]};
    const float a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const float f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2], c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
    const float b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
    const float den = a * e - b * b;
    float s = den > 1e-12f ? qa_sc_clamp01((b * f - c * e) / den) : 0.f;
    float t = (b * s + f) / e;
    if (t < 0.f) { t = 0.f; s = qa_sc_clamp01(-c / a); }
    else if (t > 1.f) { t = 1.f; s = qa_sc_clamp01((b - c) / a); }
    *s_ = s; *t_ = t;
}

// calf capsule (knee, foot) against hip capsule (h0, h1).  The operands are ordered by ROLE (calf first), not by lane: the two lanes of a
// pair call this with the same four points and agree bit for bit on everything it returns.
QA_SC_FN void qa_sc_calf_hip(const float knee[3], const float foot[3], const float h0[3], const float h1[3], qa_sc_contact *out) {
    float s, t;
    qa_sc_segment_closest(knee, foot, h0, h1, &s, &t);
    float dv[3];
    QA_SC_UNROLL
    for (int i = 0; i < 3; ++i) {
        out->pc[i] = knee[i] + s * (foot[i] - knee[i]);
        out->ph[i] = h0[i] + t * (h1[i] - h0[i]);
        dv[i] = out->pc[i] - out->ph[i];
    }
    const float dist = sqrtf(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    const float inv = dist > 1e-6f ? 1.0f / dist : 0.f;
    out->n[0] = dv[0] * inv; out->n[1] = dv[1] * inv; out->n[2] = dist > 1e-6f ? dv[2] * inv : 1.f;      // coincident axes: any unit vector
    out->gap = dist - (QA_CALF_RADIUS + s * (QA_FOOT_RADIUS - QA_CALF_RADIUS)) - QA_HIP_CAP_RADIUS;
    out->s = s; out->t = t;
}

// ---- calf against the thigh of the front / rear neighbour (qa_set_self_collision_thighs).  The thigh is the URDF's thigh box
// 0.11 x 0.0245 x 0.034 taken as its circumscribed capsule: segment (0, 0, -0.0515) .. (0, 0, -0.1615) in the thigh link's frame, radius 21 mm.
// The knee sits at (0, 0, -0.213) of that frame, so the segment lies on the line thigh joint origin -> knee at these two fractions of it.
#define QA_THIGH_CAP_RADIUS 0.021f
#define QA_THIGH_CAP_F0 (0.0515f / 0.213f)
#define QA_THIGH_CAP_F1 (0.1615f / 0.213f)

// the thigh capsule's segment from the thigh joint origin and the knee (base frame)
QA_SC_FN void qa_sc_thigh_segment(const float thigh_org[3], const float knee[3], float t0[3], float t1[3]) {
    QA_SC_UNROLL
    for (int i = 0; i < 3; ++i) {
        const float d = knee[i] - thigh_org[i];
        t0[i] = thigh_org[i] + QA_THIGH_CAP_F0 * d;
        t1[i] = thigh_org[i] + QA_THIGH_CAP_F1 * d;
    }
}

// calf capsule (knee, foot) against thigh capsule (t0, t1): qa_sc_calf_hip's expressions with the thigh's radius.  Operands by ROLE (calf first);
// in the result t, ph and n refer to the thigh where the hip's comments say hip.
QA_SC_FN void qa_sc_calf_thigh(const float knee[3], const float foot[3], const float t0[3], const float t1[3], qa_sc_contact *out) {
    float s, t;
    qa_sc_segment_closest(knee, foot, t0, t1, &s, &t);
    float dv[3];
    QA_SC_UNROLL
    for (int i = 0; i < 3; ++i) {
        out->pc[i] = knee[i] + s * (foot[i] - knee[i]);
        out->ph[i] = t0[i] + t * (t1[i] - t0[i]);
        dv[i] = out->pc[i] - out->ph[i];
    }
    const float dist = sqrtf(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    const float inv = dist > 1e-6f ? 1.0f / dist : 0.f;
    out->n[0] = dv[0] * inv; out->n[1] = dv[1] * inv; out->n[2] = dist > 1e-6f ? dv[2] * inv : 1.f;      // coincident axes: any unit vector
    out->gap = dist - (QA_CALF_RADIUS + s * (QA_FOOT_RADIUS - QA_CALF_RADIUS)) - QA_THIGH_CAP_RADIUS;
    out->s = s; out->t = t;
}

#endif
