// qa_physics.h -- one physics substep of one Go2, executed by the 4 lanes of a quad (lane = leg).
//
// Model: floating base + 4 x 3 revolute joints, all spatial quantities
// expressed in the base frame at the base origin.  Each lane builds its own leg (kinematics,
// link inertias, composite inertias, the 3x3 leg block L of the mass matrix and the 6x3
// base-coupling block F, Newton-Euler bias).  The legs only couple through the base, so
//     M = [ Mbb  F ] ,   a_leg = Linv (r_leg - F^T a_b) ,   (Mbb - sum_l F Linv F^T) a_b = r_b - sum_l F Linv r_leg
//         [ F^T  L ]
// i.e. the 18x18 solve collapses to four lane-local 3x3 inverses, a quad-sum of a 6x6 Schur
// complement (DPP), and one 6x6 SPD inverse that every lane evaluates redundantly.  Contact and
// joint-limit rows are solved by projected Gauss-Seidel in the reduced coordinates
// (u_b, w_l = u_l - G_l u_b), in which an impulse on leg l touches only u_b and w_l.
#pragma once
#include "qa_device.h"

#define QA_LEG_TBL 124           // floats per leg in the constant table
#define QA_BASE_TBL 44
#define QA_TBL_FLOATS (4 * QA_LEG_TBL + QA_BASE_TBL)
// offsets inside a leg table
#define T_HIP_ORG 0
#define T_THIGH_ORG 3
#define T_CALF_ORG 6
#define T_FOOT_ORG 9
#define T_MASS 12
#define T_COM 15
#define T_INERTIA 24
#define T_LOWER 42
#define T_UPPER 45
#define T_EFFORT 48
#define T_VELLIM 51
#define T_POINTS 54              // 17 x (x y z r); point 0 is the foot sphere
#define QA_LEG_PTS 17
#define QA_BASE_PTS 11

#define QA_LIMIT_MARGIN 0.2f     // rad: beyond 30.1 rad/s x 5 ms = 0.15 rad a stop cannot bind within one substep
#define QA_LIMIT_DEPEN 1.0f      // rad/s
#define QA_CFM 1e-6f
#define QA_OPEN_BIAS 1e30f      // bias of a row whose contact is open: the residual stays positive, the impulse stays 0

struct PhysParams {
    float dt, gz, contact_offset, max_depen, ground_friction;
    int iters;
    int slots;     // extra contact slots per leg: 3 (one per body) or 1 (lowest non-foot point only)
    int self_collision;   // calf capsules of neighbouring legs collide (cfg.self_collision)
};

// packed lower-triangular index of a symmetric 6x6
#define SIDX(i, j) ((i) >= (j) ? ((i) * ((i) + 1) / 2 + (j)) : ((j) * ((j) + 1) / 2 + (i)))

// inverse of a symmetric positive definite 6x6 given packed (21); Cholesky + triangular inverse
QA_DEV void spd6_inverse(const float *A, float *Ainv) {
    float Lc[21];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float d = A[SIDX(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= Lc[SIDX(j, k)] * Lc[SIDX(j, k)];
        float inv = rsqrtf(d);
        Lc[SIDX(j, j)] = inv;                 // store 1/L_jj on the diagonal
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float s = A[SIDX(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= Lc[SIDX(i, k)] * Lc[SIDX(j, k)];
            Lc[SIDX(i, j)] = s * inv;
        }
    }
    // T = L^-1 (lower triangular), column by column
    float T[21];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        T[SIDX(j, j)] = Lc[SIDX(j, j)];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float s = 0.f;
#pragma unroll
            for (int k = j; k < i; ++k) s -= Lc[SIDX(i, k)] * T[SIDX(k, j)];
            T[SIDX(i, j)] = s * Lc[SIDX(i, i)];
        }
    }
    // A^-1 = T^T T
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = i; k < 6; ++k) s += T[SIDX(k, i)] * T[SIDX(k, j)];
            Ainv[SIDX(i, j)] = s;
        }
}

QA_DEV void sym6_mul(const float *A, const float *x, float *y) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) s = fmaf(A[SIDX(i, j)], x[j], s);
        y[i] = s;
    }
}

// Terrain under an env: a 16 x 16 window of height samples (metres) staged in LDS once per env step, centred on the
// base.  Leg points reach < 0.6 m from the base origin and the base moves < 0.1 m per env step, so every contact
// query of the 4 substeps falls inside the window (+-0.8 m); indices are clamped regardless.
#define QA_PATCH 16
struct TerrainView {
    const float *patch;      // LDS, QA_PATCH x QA_PATCH, row-major (x major), metres
    const int16_t *samples;  // the whole field in HBM (fallback for queries outside the window)
    const int16_t *ceil;     // undersides of overhangs on the same grid (QA_T_CEILING_SAMPLES), nullptr = none
    int ix0, iy0;            // global cell of patch[0][0]
    int rows, cols;
    float border, hscale, inv_hscale, vscale;
    // r5: ENV-LOCAL horizontal coordinates inside a step.  The root's world (x, y) at the start of the step is the ANCHOR; the substeps
    // integrate and query the terrain with offsets from it (|offset| < 1 m: one fp32 ulp is 6e-8 m instead of the 6e-5 m it is 900 m
    // from the origin, where the 8192-env course puts its last envs -- VERDICT r4 item 6: 3.7 % of those env-steps flipped a contact on
    // exactly that).  The anchor's cell and its fraction of a cell are computed ONCE per env step in double: cell of a point at offset
    // dx = cax + floor(fax + dx / hscale).  The oracle works in double in world coordinates and needs none of this.
    int cax, cay;            // cell of the anchor
    float fax, fay;          // the anchor's position inside its cell, [0, 1)
    float ancx, ancy;        // the anchor (world): obstacle centres are re-expressed relative to it when they are staged
    // articulated course obstacles of this env (cfg.articulated_obstacles): LDS record of QA_OBST_PER_ENV x 12 floats
    // [QA_T_OBST_DESC row (8) | q, q_dot, -, damping] and, when the caller integrates the obstacle joints, 3 force accumulators
    const float *ob;         // nullptr = none
    float *ob_acc;           // nullptr = contact forces are not accumulated (single substeps: qa_simulate)
};
// the anchor of a step = the root's world (x, y) at its start; and the terrain window centred on it
QA_DEV void set_anchor(TerrainView &T, float x, float y) {
    const double ax = ((double)x + (double)T.border) / (double)T.hscale, ay = ((double)y + (double)T.border) / (double)T.hscale;
    const double cx = floor(ax), cy = floor(ay);
    T.cax = (int)cx; T.cay = (int)cy; T.fax = (float)(ax - cx); T.fay = (float)(ay - cy); T.ancx = x; T.ancy = y;
}
QA_DEV void patch_origin(TerrainView &T, float x, float y) {
    set_anchor(T, x, y);
    T.ix0 = max(min(T.cax - (QA_PATCH / 2 - 1), T.rows - QA_PATCH), 0);
    T.iy0 = max(min(T.cay - (QA_PATCH / 2 - 1), T.cols - QA_PATCH), 0);
}
// cell (clamped to the field) and position inside it of the point at offset (dx, dy) from the anchor
QA_DEV void anchor_cell(const TerrainView &T, float dx, float dy, int &ix, int &iy, float &u, float &v) {
    const float fx = fmaf(dx, T.inv_hscale, T.fax), fy = fmaf(dy, T.inv_hscale, T.fay);
    const float flx = floorf(fx), fly = floorf(fy);
    const int gx = T.cax + (int)flx, gy = T.cay + (int)fly;
    ix = min(max(gx, 0), T.rows - 2); iy = min(max(gy, 0), T.cols - 2);
    u = clampf(fx - flx + (float)(gx - ix), 0.f, 1.f); v = clampf(fy - fly + (float)(gy - iy), 0.f, 1.f);
}
// the quad of an env fills its window: lane `leg` loads rows 4 leg .. 4 leg + 3
QA_DEV void stage_patch(const TerrainView &T, float *patch, int leg) {
#pragma unroll
    for (int r = 0; r < QA_PATCH / 4; ++r) {
        const int lx = 4 * leg + r, gx = min(T.ix0 + lx, T.rows - 1);
        const int16_t *src = T.samples + (int64_t)gx * T.cols;
        int16_t v[QA_PATCH];
#pragma unroll
        for (int j = 0; j < QA_PATCH; ++j) v[j] = src[min(T.iy0 + j, T.cols - 1)];
#pragma unroll
        for (int j = 0; j < QA_PATCH; ++j) patch[lx * QA_PATCH + j] = (float)v[j] * T.vscale;
    }
}
// height and unit normal of the terrain under the point at offset (x, y) from the step's anchor: two triangles per cell, split along (i,j)-(i+1,j+1)
QA_DEV void ground_query(const TerrainView &T, float x, float y, float &h, V3 &n) {
    int ix, iy; float u, v;
    anchor_cell(T, x, y, ix, iy, u, v);
    int lx = ix - T.ix0, ly = iy - T.iy0;
    float h00, h01, h10, h11;
    if ((unsigned)lx <= QA_PATCH - 2 && (unsigned)ly <= QA_PATCH - 2) {
        const float *c = T.patch + lx * QA_PATCH + ly;
        h00 = c[0]; h01 = c[1]; h10 = c[QA_PATCH]; h11 = c[QA_PATCH + 1];
    } else {        // outside the window (a fully stretched leg at the window edge): read the field itself
        const int16_t *g = T.samples + (int64_t)ix * T.cols + iy;
        h00 = (float)g[0] * T.vscale; h01 = (float)g[1] * T.vscale; h10 = (float)g[T.cols] * T.vscale; h11 = (float)g[T.cols + 1] * T.vscale;
    }
    float gx, gy;
    if (u >= v) { gx = h10 - h00; gy = h11 - h10; h = h00 + u * gx + v * gy; }
    else { gy = h01 - h00; gx = h11 - h01; h = h00 + v * gy + u * gx; }
    gx *= T.inv_hscale; gy *= T.inv_hscale;
    float inv = rsqrtf(gx * gx + gy * gy + 1.0f);
    n = v3(-gx * inv, -gy * inv, inv);
}
// Gap and contact normal of a sphere (centre (x, y, zw), radius r) against the terrain: the plane of the floor triangle under it or,
// where QA_T_CEILING_SAMPLES has one and it is nearer, of the ceiling triangle above it (tunnel roof, upper arc of the tyre).  A
// triangle with a QA_NO_CEILING corner does not exist; the ceiling's normal points down.  Ceiling samples are read from HBM (an
// env is under an overhang for a few steps of an episode; the floor window in LDS is what every query needs).
// `vs`: velocity of the contacted surface along n (articulated obstacles move: the normal row's bias is gap/dt - vs), `ca`: d vs / d q_dot of
// the obstacle joint (the contact's generalised force on that joint is -f_n ca), `ob`: the obstacle slot, -1 = fixed terrain.
// Inside the see-saw's footprint the height map's static tent is replaced by {flat ground, the plank's top plane through the pivot at
// tilt q}; inside the bar's / tyre's footprint the map (and the tyre's ceiling arc) is shifted vertically by the joint offset q.
QA_DEV float contact_query(const TerrainView &T, float x, float y, float zw, float r, V3 &n, float &vs, float &ca, int &ob) {
    vs = 0.f; ca = 0.f; ob = -1;
    int mode = 0, slot = -1;                      // 1 = see-saw footprint, 2 = shifted map
    float xl = 0.f, cpsi = 1.f, spsi = 0.f, oq = 0.f, oqd = 0.f, oh0 = 0.f;
    if (T.ob) {
#pragma unroll
        for (int k = 0; k < QA_OBST_PER_ENV; ++k) {
            const float *d = T.ob + 12 * k;
            const float kind = d[7];
            const float dx = x - d[0], dy = y - d[1];
            const float lx = d[2] * dx + d[3] * dy, ly = d[2] * dy - d[3] * dx;
            if (kind != 0.f && fabsf(lx) <= d[4] && fabsf(ly) <= d[5]) {
                mode = kind == (float)QA_OBST_SEESAW ? 1 : 2; slot = k; xl = lx; cpsi = d[2]; spsi = d[3]; oh0 = d[6]; oq = d[8]; oqd = d[9];
            }
        }
    }
    const float zq = mode == 2 ? zw - oq : zw;      // a surface raised by q == the point lowered by q
    float gh; ground_query(T, x, y, gh, n);
    float gap = (zq - gh) * n.z - r;
    if (T.ceil) {
        int ix, iy; float u, v;
        anchor_cell(T, x, y, ix, iy, u, v);
        const int16_t *g = T.ceil + (int64_t)ix * T.cols + iy;
        const int s00 = g[0], s01 = g[1], s10 = g[T.cols], s11 = g[T.cols + 1];
        const bool lower = u >= v;                       // triangle (00, 10, 11), else (00, 01, 11)
        const bool exists = s00 != QA_NO_CEILING && s11 != QA_NO_CEILING && (lower ? s10 : s01) != QA_NO_CEILING;
        const float h00 = (float)s00 * T.vscale, h01 = (float)s01 * T.vscale, h10 = (float)s10 * T.vscale, h11 = (float)s11 * T.vscale;
        float gx = lower ? h10 - h00 : h11 - h01, gy = lower ? h11 - h10 : h01 - h00;
        const float ch = h00 + u * gx + v * gy;
        gx *= T.inv_hscale; gy *= T.inv_hscale;
        const float inv = rsqrtf(gx * gx + gy * gy + 1.0f), cgap = (ch - zq) * inv - r;
        // thin shell: acts on points below it or at most QA_CEILING_SHELL above it, and only where it lies above the floor map
        if (exists && ch > gh && (ch - zq) * inv >= -QA_CEILING_SHELL && cgap < gap) { gap = cgap; n = v3(gx * inv, gy * inv, -inv); }
    }
    if (mode == 2) { ca = n.z; vs = n.z * oqd; ob = slot; }
    else if (mode == 1) {
        float sq, cq; __sincosf(oq, &sq, &cq);
        const float zl = zw - oh0, pgap = xl * sq + zl * cq - r;         // distance to the plank's top plane, normal (sin q, 0, cos q) in the obstacle frame
        gap = zw - r; n = v3(0.f, 0.f, 1.f);                             // the ground under the see-saw (the map's tent is not collided with)
        if (pgap >= -QA_SEESAW_SHELL && pgap < gap) {
            gap = pgap; n = v3(cpsi * sq, spsi * sq, cq);
            ca = sq * zl - cq * xl; vs = ca * oqd;                        // n . (q_dot y' x r), r from the pivot
            ob = slot;
        }
    }
    return gap;
}
QA_DEV float contact_query(const TerrainView &T, float x, float y, float zw, float r, V3 &n) {
    float vs, ca; int ob;
    return contact_query(T, x, y, zw, r, n, vs, ca, ob);
}
// legged_robot.py:1209-1228 for the one scan point the BBC env consumes: (0, 0.1) in the yaw frame, truncated to a
// cell, min of three samples.  Integer samples are read from HBM (one env-step-level lookup per quad).
QA_DEV float scan_center_height(const TerrainView &T, V3 pos, float qz, float qw) {
    float nrm = fmaxf(sqrtf(qz * qz + qw * qw), 1e-9f);
    qz /= nrm; qw /= nrm;
    const float vx = 0.0f, vy = 0.1f;
    float tx = -qz * vy * 2.0f, ty = qz * vx * 2.0f;
    float px = vx + qw * tx - qz * ty + pos.x, py = vy + qw * ty + qz * tx + pos.y;
    px += T.border; py += T.border;
    int ix = (int)(px / T.hscale), iy = (int)(py / T.hscale);
    ix = min(max(ix, 0), T.rows - 2); iy = min(max(iy, 0), T.cols - 2);
    const int16_t *g = T.samples + (int64_t)ix * T.cols + iy;
    int a = g[0], b = g[T.cols], d = g[1];
    int m = min(min(a, b), d);
    return (float)m * T.vscale;
}
// tangent basis of a contact: t1 = world x projected onto the tangent plane, t2 = n x t1
QA_DEV void tangent_basis(V3 n, V3 &t1, V3 &t2) {
    V3 a = v3(1.0f - n.x * n.x, -n.x * n.y, -n.x * n.z);
    t1 = rsqrtf(dot(a, a)) * a;
    t2 = cross(n, t1);
}

// state of one env as seen by one lane (registers)
struct EnvState {
    V3 pos; float qx, qy, qz, qw; V3 vw, ww;    // root, replicated across the quad
    float q[3], qd[3];                          // this lane's leg
};

// Non-foot contacts of a leg: one CANDIDATE per body group -- group 0 = the hip link or this lane's share of the base / head
// points (whichever point is lowest), group 1 = thigh, group 2 = calf -- so that thigh and calf (the bodies _reward_collision
// counts) and hip / base (the bodies check_termination reads) can report forces independently.  Up to QA_EXTRA_SLOTS = 2 of the
// three candidates make contact in a substep (all three inside the contact offset: the one with the largest gap waits); the
// active ones are compacted into slots 0..1 per lane, so a wavefront pays for max-over-lanes(#active), not for every group
// that is active somewhere in it.
#define QA_EXTRA_GROUPS 3
#define QA_EXTRA_SLOTS 2
struct ContactOut {
    V3 foot_f;                      // world-frame force on this leg's foot
    V3 extra_f[QA_EXTRA_SLOTS];     // world-frame force on the slot's contact
    int extra_body[QA_EXTRA_SLOTS]; // body id the slot's contact is on (-1 none)
    V3 self_f;                      // world-frame force of this leg's self-collisions (both partners), on its calf
    // SCH instantiations only (calf against the neighbouring hip): the row's impulse of this substep (0 while the pair is apart) and the world-frame
    // direction of its force on THIS leg's body -- the calf of a front leg, the hip of a rear leg.  The kernels turn them into a force behind
    // phys_substep: the block below that reports the other forces stays the same code with and without the rows
    float sh_lam; V3 sh_dir;
    // SCH = 2 only (calf against the front / rear neighbour's thigh): the same pair of values per row -- row 0 is the front leg's calf on the rear
    // leg's thigh, row 1 the rear leg's calf on the front leg's thigh; the direction is that of the force on THIS leg's calf or thigh
    float st_lam[2]; V3 st_dir[2];
};

// Self-collision (the reference enables it: bbc/.../go2_locomotion_config.py:72, tsc/.../go2_agility_config.py:43 `self_collisions = 0`): the
// lower legs as capsules -- knee to foot centre, radius QA_CALF_RADIUS at the knee growing to the foot sphere's -- tested against the
// capsules of the left/right neighbour (lane ^ 1) and of the front/rear neighbour (lane ^ 2): the pairs that can meet under the joint
// limits (a leg cannot reach its diagonal partner, and the thigh / trunk pairs are out of reach of the calf's -0.84 rad upper stop).
// One frictionless row per pair at the capsules' closest points.  The two points move with the SAME base, so the row has no base
// Jacobian of its own (n is along pA - pB): in the reduced coordinates it is jl_A . w_A - jl_B . w_B + (G_A^T jl_A - G_B^T jl_B) . u_b.
#define QA_CALF_RADIUS 0.013f
#define QA_FOOT_RADIUS 0.022f
#define QA_PRIV_SELF 140                 // 2 pair rows x 20 floats
// The calf of a front leg against the hip of the rear leg of its side (SCH instantiations, include/qa_sim_selfcol.h): the one ordered relation
// that can come within the contact offset under the joint limits.  Same algebra as above, with chain depth 3 on the calf's
// side and 1 on the hip's (only joint 0 moves the hip cylinder).  Geometry: qa_selfcol.h, shared with the host twin.
#include "qa_selfcol.h"
// closest points of segments A0 + s (A1 - A0), B0 + t (B1 - B0), s, t in [0, 1] (Ericson, Real-Time Collision Detection 5.1.9)
QA_DEV void segment_closest(V3 A0, V3 A1, V3 B0, V3 B1, float &s, float &t) {
    const V3 d1 = A1 - A0, d2 = B1 - B0, r = A0 - B0;
    const float a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
    const float den = a * e - b * b;
    s = den > 1e-12f ? clampf((b * f - c * e) / den, 0.f, 1.f) : 0.f;
    t = (b * s + f) / e;
    if (t < 0.f) { t = 0.f; s = clampf(-c / a, 0.f, 1.f); }
    else if (t > 1.f) { t = 1.f; s = clampf((b - c) / a, 0.f, 1.f); }
}

// one scalar constraint row in reduced coordinates
struct Row {
    float jh[6];   // J_b + G^T j_l
    float jl[3];
    float bj[6];   // Binv jh
    float lj[3];   // Linv jl
    float dinv, bias, lam;
};

QA_DEV void row_finish(Row &r, const float *G, const float *Linv, const float *Binv, const float *jb) {
#pragma unroll
    for (int i = 0; i < 6; ++i) r.jh[i] = jb[i] + G[0 * 6 + i] * r.jl[0] + G[1 * 6 + i] * r.jl[1] + G[2 * 6 + i] * r.jl[2];
    sym6_mul(Binv, r.jh, r.bj);
    // Linv packed: 00 01 02 11 12 22
    r.lj[0] = Linv[0] * r.jl[0] + Linv[1] * r.jl[1] + Linv[2] * r.jl[2];
    r.lj[1] = Linv[1] * r.jl[0] + Linv[3] * r.jl[1] + Linv[4] * r.jl[2];
    r.lj[2] = Linv[2] * r.jl[0] + Linv[4] * r.jl[1] + Linv[5] * r.jl[2];
    float d = r.jl[0] * r.lj[0] + r.jl[1] * r.lj[1] + r.jl[2] * r.lj[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) d = fmaf(r.jh[i], r.bj[i], d);
    r.dinv = 1.0f / (d + QA_CFM);
    r.lam = 0.f;
}

// residual of a row with three independent partial sums (short dependency chains: one wave per SIMD has no
// other wave to hide VALU latency behind)
QA_DEV float row_residual(const Row &r, const float *ub, const float *w) {
    float a = fmaf(r.jh[2], ub[2], fmaf(r.jh[1], ub[1], r.jh[0] * ub[0]));
    float b = fmaf(r.jh[5], ub[5], fmaf(r.jh[4], ub[4], r.jh[3] * ub[3]));
    float c = fmaf(r.jl[2], w[2], fmaf(r.jl[1], w[1], r.jl[0] * w[0]));
    return (a + b) + (c + r.bias);
}
// Gauss-Seidel update of one contact on the lane-local copy (ub, w): normal row, then the two tangent rows
// TOGETHER from the velocity the normal row left (pyramid friction |lam_t| <= mu lam_n)
QA_DEV void contact_update(Row *r, float *ub, float *w, float mu) {
    {
        float lam = fmaxf(r[0].lam - row_residual(r[0], ub, w) * r[0].dinv, 0.f);
        float dl = lam - r[0].lam;
        r[0].lam = lam;
#pragma unroll
        for (int i = 0; i < 6; ++i) ub[i] = fmaf(r[0].bj[i], dl, ub[i]);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = fmaf(r[0].lj[k], dl, w[k]);
    }
    const float lim = mu * r[0].lam;
    float l1 = clampf(r[1].lam - row_residual(r[1], ub, w) * r[1].dinv, -lim, lim);
    float l2 = clampf(r[2].lam - row_residual(r[2], ub, w) * r[2].dinv, -lim, lim);
    float d1 = l1 - r[1].lam, d2 = l2 - r[2].lam;
    r[1].lam = l1; r[2].lam = l2;
#pragma unroll
    for (int i = 0; i < 6; ++i) ub[i] = fmaf(r[2].bj[i], d2, fmaf(r[1].bj[i], d1, ub[i]));
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = fmaf(r[2].lj[k], d2, fmaf(r[1].lj[k], d1, w[k]));
}

// build the three rows (normal, tangent1, tangent2) of a contact at base-frame point p of chain depth `depth`
QA_DEV void contact_rows(Row *rows, V3 p, int depth, float gap, const V3 *o, const V3 *ax, V3 nB, V3 t1B, V3 t2B,
                         const float *G, const float *Linv, const float *Binv, const PhysParams &P) {
    V3 dirs[3] = {nB, t1B, t2B};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        V3 pxd = cross(p, dirs[d]);
        float jb[6] = {pxd.x, pxd.y, pxd.z, dirs[d].x, dirs[d].y, dirs[d].z};
#pragma unroll
        for (int k = 0; k < 3; ++k) rows[d].jl[k] = (k < depth) ? dot(dirs[d], cross(ax[k], p - o[k])) : 0.f;
        row_finish(rows[d], G, Linv, Binv, jb);
        rows[d].bias = 0.f;
    }
    float g = gap / P.dt;
    rows[0].bias = gap >= 0.f ? g : fmaxf(g, -P.max_depen);
}

// ---------------------------------------------------------------------------------------------
// One substep.  tbl = this lane's leg table (LDS), btbl = base point table (LDS), binert = base
// link inertia (10 floats), tau = joint torques of this leg (already clipped), mu = friction.
// Returns contact forces; updates st in place.  If fk_out != nullptr, writes the joint origins
// and the foot origin of the NEW state in the base frame (4 points) for RIGID_BODY_POS.
// development aid: -DQA_SUBPROF adds s_memtime stamps of the substep's sections (tools/substep_profile.py builds its own
// copy of the library with it; the product build has none of this)
#ifdef QA_SUBPROF
#ifndef QA_SUBPROF_PTR
#define QA_SUBPROF_PTR g_subprof         // qa_sim.hip gives each of its translation units a name of its own
#endif
__device__ long long *QA_SUBPROF_PTR = nullptr;
#define QA_SUBSTAMP(k) do { __builtin_amdgcn_sched_barrier(0); if (QA_SUBPROF_PTR && threadIdx.x == 0) QA_SUBPROF_PTR[blockIdx.x * 32 + 16 + (k)] = (long long)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define QA_SUBSTAMP(k) do { } while (0)
#endif

// rarely-active rows live in per-lane LDS slots: slot k of this lane is priv[k * QA_PRIV_STRIDE]
#define QA_PRIV_STRIDE 64
#define QA_PRIV_EXTRA 0                  // 2 slots x 3 rows x 20 floats: jh6 jl3 bj6 lj3 dinv bias
#define QA_PRIV_STEP 120                 // env-step persistents parked between substeps: act3 sp3 sd3 binert10
#define QA_PRIV_FLOATS 180
#define QA_PRIV_HIPS 180                 // SCH instantiations: 1 calf-hip row x 20 floats behind the records above ...
#define QA_PRIV_FLOATS_SCH 204           // ... and a lane stride that is again an odd number of 16-byte records (51)
#define QA_PRIV_THIGHS 200               // SCH = 2: 2 calf-thigh rows x 20 floats behind the calf-hip row ...
#define QA_PRIV_FLOATS_SCT 244           // ... lane stride 61 records, odd again
#define QA_PRIV_FLOATS_OF(SCH) ((SCH) >= 2 ? QA_PRIV_FLOATS_SCT : (SCH) ? QA_PRIV_FLOATS_SCH : QA_PRIV_FLOATS)
struct LRow { float *p; };               // row view in LDS
QA_DEV float &lr(float *priv, int k) { return priv[k * QA_PRIV_STRIDE]; }

QA_DEV void row_store(float *priv, int base, const Row &r) {
#pragma unroll
    for (int i = 0; i < 6; ++i) { lr(priv, base + i) = r.jh[i]; lr(priv, base + 9 + i) = r.bj[i]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lr(priv, base + 6 + k) = r.jl[k]; lr(priv, base + 15 + k) = r.lj[k]; }
    lr(priv, base + 18) = r.dinv; lr(priv, base + 19) = r.bias;
}
QA_DEV void row_load(float *priv, int base, Row &r) {
#pragma unroll
    for (int i = 0; i < 6; ++i) { r.jh[i] = lr(priv, base + i); r.bj[i] = lr(priv, base + 9 + i); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.jl[k] = lr(priv, base + 6 + k); r.lj[k] = lr(priv, base + 15 + k); }
    r.dinv = lr(priv, base + 18); r.bias = lr(priv, base + 19);
}

// ---------------------------------------------------------------------------------------------
// r5: the constraint rows and the Gauss-Seidel sweeps in PACKED fp32 (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32).
// Why (tools/valu_rate.hip, profiles/r5_valu_issue_rate.txt): at 4096 envs the kernel is ONE wavefront per CU, and a wavefront alone
// on a SIMD issues one VALU instruction per ~4.5 cycles whether the next one depends on it or not and whether it is v_fma_f32 or
// v_pk_fma_f32 -- so the time is the instruction count and a packed instruction carries two FMAs in one issue slot.  A row is
//     j = (jh0 jh1 | jh2 jh3 | jh4 jh5 | jl0 jl1 | jl2 bias),   m = (bj0 bj1 | bj2 bj3 | bj4 bj5 | lj0 lj1 | lj2 0)
// against the state x = (ub0 ub1 | ub2 ub3 | ub4 ub5 | w0 w1 | w2 1): residual = sum of both halves of sum_i j_i x_i (5 packed ops + 2),
// update x_i += m_i dl (5 packed ops) -- 15 instructions per row instead of 25.  The SLP vectoriser is still off for this file (its
// ad-hoc packing costs more moves than it saves, __graft_entry__.py); here the data is laid out in pairs from the start.
// (the round-4 scalar rows and sweeps, 85 us against 69 us per launch, were removed in r6: profiles/r5_env_step_packed_vs_scalar.txt has the A/B.)
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
QA_DEV f2 f2s(float s) { return f2{s, s}; }
QA_DEV f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
QA_DEV float hsum(f2 a) { return a.x + a.y; }
struct PRow { f2 j[5]; f2 m[5]; float dinv, lam; };
// what the rows of a substep are built from, in pairs: G2[k][p] = (G[k][2p], G[k][2p+1]); Bc[p][c] = (Binv[2p][c], Binv[2p+1][c]);
// L01[k] = (Linv[0][k], Linv[1][k]), L2[k] = Linv[2][k]
struct PSolve { f2 G2[3][3]; f2 Bc[3][6]; f2 L01[3]; float L2[3]; };
QA_DEV void psolve_make(PSolve &S, const float *G, const float *Linv, const float *Binv) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int q = 0; q < 3; ++q) S.G2[k][q] = f2{G[k * 6 + 2 * q], G[k * 6 + 2 * q + 1]};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int c = 0; c < 6; ++c) S.Bc[q][c] = f2{Binv[SIDX(2 * q, c)], Binv[SIDX(2 * q + 1, c)]};
    // Linv packed: 00 01 02 11 12 22
    S.L01[0] = f2{Linv[0], Linv[1]}; S.L01[1] = f2{Linv[1], Linv[3]}; S.L01[2] = f2{Linv[2], Linv[4]};
    S.L2[0] = Linv[2]; S.L2[1] = Linv[4]; S.L2[2] = Linv[5];
}
// bj = Binv jh, two accumulators per output pair (one wave per SIMD: short chains)
QA_DEV void pbinv_mul(const PSolve &S, const f2 *jh, f2 *bj) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        f2 a = S.Bc[q][0] * f2s(jh[0].x), b = S.Bc[q][1] * f2s(jh[0].y);
        a = pfma(S.Bc[q][2], f2s(jh[1].x), a); b = pfma(S.Bc[q][3], f2s(jh[1].y), b);
        a = pfma(S.Bc[q][4], f2s(jh[2].x), a); b = pfma(S.Bc[q][5], f2s(jh[2].y), b);
        bj[q] = a + b;
    }
}
QA_DEV void prow_finish(PRow &r, const PSolve &S, const float *jb, const float *jl, float bias) {
    f2 jh[3], bj[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        jh[q] = pfma(S.G2[2][q], f2s(jl[2]), pfma(S.G2[1][q], f2s(jl[1]), pfma(S.G2[0][q], f2s(jl[0]), f2{jb[2 * q], jb[2 * q + 1]})));
    pbinv_mul(S, jh, bj);
    const f2 lj01 = pfma(S.L01[2], f2s(jl[2]), pfma(S.L01[1], f2s(jl[1]), S.L01[0] * f2s(jl[0])));
    const float lj2 = fmaf(S.L2[2], jl[2], fmaf(S.L2[1], jl[1], S.L2[0] * jl[0]));
    const f2 jl01 = f2{jl[0], jl[1]};
    f2 dd = pfma(jh[1], bj[1], jh[0] * bj[0]), de = pfma(jl01, lj01, jh[2] * bj[2]);
    const float d = fmaf(jl[2], lj2, hsum(dd + de));
    r.dinv = 1.0f / (d + QA_CFM);
    r.lam = 0.f;
    r.j[0] = jh[0]; r.j[1] = jh[1]; r.j[2] = jh[2]; r.j[3] = jl01; r.j[4] = f2{jl[2], bias};
    r.m[0] = bj[0]; r.m[1] = bj[1]; r.m[2] = bj[2]; r.m[3] = lj01; r.m[4] = f2{lj2, 0.f};
}
QA_DEV float prow_residual(const PRow &r, const f2 *x) {
    f2 a = r.j[0] * x[0], b = r.j[1] * x[1];
    a = pfma(r.j[2], x[2], a); b = pfma(r.j[3], x[3], b); a = pfma(r.j[4], x[4], a);
    return hsum(a + b);
}
// Gauss-Seidel update of one contact on the lane-local state x: normal row, then the two tangent rows TOGETHER from the velocity the normal
// row left (pyramid friction |lam_t| <= mu lam_n) -- contact_update() in pairs
QA_DEV void pcontact_update(PRow *r, f2 *x, float mu) {
    {
        const float lam = fmaxf(fmaf(-prow_residual(r[0], x), r[0].dinv, r[0].lam), 0.f);
        const f2 dl = f2s(lam - r[0].lam);
        r[0].lam = lam;
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = pfma(r[0].m[i], dl, x[i]);
    }
    const float lim = mu * r[0].lam;
    const float l1 = clampf(fmaf(-prow_residual(r[1], x), r[1].dinv, r[1].lam), -lim, lim);
    const float l2 = clampf(fmaf(-prow_residual(r[2], x), r[2].dinv, r[2].lam), -lim, lim);
    const f2 d1 = f2s(l1 - r[1].lam), d2 = f2s(l2 - r[2].lam);
    r[1].lam = l1; r[2].lam = l2;
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = pfma(r[2].m[i], d2, pfma(r[1].m[i], d1, x[i]));
}
// the three rows (normal, tangent 1, tangent 2) of a contact at base-frame point p of chain depth `depth` -- contact_rows() in pairs
QA_DEV void pcontact_rows(PRow *rows, V3 p, int depth, float gap, float vs, const V3 *o, const V3 *ax, V3 nB, V3 t1B, V3 t2B, const PSolve &S, const PhysParams &P) {
    const V3 dirs[3] = {nB, t1B, t2B};
    V3 lever[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lever[k] = cross(ax[k], p - o[k]);
    const float g = gap / P.dt;
    const float bias0 = (gap >= 0.f ? g : fmaxf(g, -P.max_depen)) - vs;        // a surface that moves along the normal (articulated obstacle): - vs
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const V3 pxd = cross(p, dirs[d]);
        const float jb[6] = {pxd.x, pxd.y, pxd.z, dirs[d].x, dirs[d].y, dirs[d].z};
        float jl[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) jl[k] = (k < depth) ? dot(dirs[d], lever[k]) : 0.f;
        prow_finish(rows[d], S, jb, jl, d == 0 ? bias0 : 0.f);
    }
}
// A lane's private LDS region is CONTIGUOUS in the packed build (QA_PRIV_FLOATS floats per lane, 16-byte records, every access a
// ds_read_b128 / ds_write_b128: lane stride 180 dwords = 45 x 16 B puts the 16 lanes of a b128 service group on 16 different bank
// quads) -- one wave alone pays ~10 cycles of issue per LDS instruction whatever its width (tools/valu_rate.hip), so a row is 5 reads
// instead of 20.  Record of a row: j0 j1 | j2 j3 | j4 m0 | m1 m2 | m3 (m4.x, dinv).
QA_DEV void prow_store(float *rec, const PRow &r) {
    f4 *q = reinterpret_cast<f4 *>(rec);
    q[0] = f4{r.j[0].x, r.j[0].y, r.j[1].x, r.j[1].y}; q[1] = f4{r.j[2].x, r.j[2].y, r.j[3].x, r.j[3].y};
    q[2] = f4{r.j[4].x, r.j[4].y, r.m[0].x, r.m[0].y}; q[3] = f4{r.m[1].x, r.m[1].y, r.m[2].x, r.m[2].y};
    q[4] = f4{r.m[3].x, r.m[3].y, r.m[4].x, r.dinv};
}
QA_DEV void prow_load(const float *rec, PRow &r) {
    const f4 *q = reinterpret_cast<const f4 *>(rec);
    const f4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    r.j[0] = f2{a.x, a.y}; r.j[1] = f2{a.z, a.w}; r.j[2] = f2{b.x, b.y}; r.j[3] = f2{b.z, b.w}; r.j[4] = f2{c.x, c.y};
    r.m[0] = f2{c.z, c.w}; r.m[1] = f2{d.x, d.y}; r.m[2] = f2{d.z, d.w}; r.m[3] = f2{e.x, e.y}; r.m[4] = f2{e.z, 0.f}; r.dinv = e.w;
}
template <int SCH = 0>
QA_DEV float *priv_of(float *s_priv, int tix) { return s_priv + tix * QA_PRIV_FLOATS_OF(SCH); }
// the reported force of the calf-hip row (SCH): +n on the front leg's calf (body 5 + 4 leg), -n on the rear leg's hip (body 3 + 4 leg)
QA_DEV void sch_forces(const ContactOut &co, float dt, int leg, V3 &hip_f, V3 &calf_f) {
    const V3 f = (co.sh_lam * (1.0f / dt)) * co.sh_dir;
    const bool calf = (leg & 2) == 0;
    // selects, not "+ 0": -0.0 + 0.0 is +0.0, and with no pair in reach the exported forces are to keep every bit
    const V3 h = hip_f + f, c = calf_f + f;
    hip_f = calf ? hip_f : h;
    calf_f = calf ? c : calf_f;
}
// the reported forces of the two calf-thigh rows (SCH = 2): +n on the calf (body 5 + 4 leg) of the row's calf leg, -n on the THIGH (body 4 + 4 leg)
// of the other leg.  A row that carried no impulse leaves both forces untouched, bit for bit.
QA_DEV void sct_forces(const ContactOut &co, float dt, int leg, V3 &thigh_f, V3 &calf_f) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const V3 f = (co.st_lam[r] * (1.0f / dt)) * co.st_dir[r];
        const bool live = co.st_lam[r] != 0.f, calf = ((leg & 2) == 0) == (r == 0);
        const V3 t = thigh_f + f, c = calf_f + f;
        thigh_f = (live && !calf) ? t : thigh_f;
        calf_f = (live && calf) ? c : calf_f;
    }
}
// One frictionless row between two bodies of a front / rear pair of legs (lane ^ 2), from this lane's joint Jacobian jl of the row: the algebra of
// the calf-calf and calf-hip rows (no base Jacobian of its own; base part and effective mass summed over the two lanes), stored as a packed record.
QA_DEV void pair_row_store(float *rec, const float jl[3], const float *G, const float *Linv, const float *Binv, float gap, float dt, float max_depen) {
    Row r;
    float h[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) h[i] = G[0 * 6 + i] * jl[0] + G[1 * 6 + i] * jl[1] + G[2 * 6 + i] * jl[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) r.jh[i] = h[i] + dpp_f<0x4E>(h[i]);
    sym6_mul(Binv, r.jh, r.bj);
    r.lj[0] = Linv[0] * jl[0] + Linv[1] * jl[1] + Linv[2] * jl[2];
    r.lj[1] = Linv[1] * jl[0] + Linv[3] * jl[1] + Linv[4] * jl[2];
    r.lj[2] = Linv[2] * jl[0] + Linv[4] * jl[1] + Linv[5] * jl[2];
    const float dleg = jl[0] * r.lj[0] + jl[1] * r.lj[1] + jl[2] * r.lj[2];
    float d = dleg + dpp_f<0x4E>(dleg);
#pragma unroll
    for (int i = 0; i < 6; ++i) d = fmaf(r.jh[i], r.bj[i], d);
    const float g = gap / dt;
    PRow pr_;
    pr_.j[0] = f2{r.jh[0], r.jh[1]}; pr_.j[1] = f2{r.jh[2], r.jh[3]}; pr_.j[2] = f2{r.jh[4], r.jh[5]}; pr_.j[3] = f2{jl[0], jl[1]};
    pr_.j[4] = f2{jl[2], gap >= 0.f ? g : fmaxf(g, -max_depen)};
    pr_.m[0] = f2{r.bj[0], r.bj[1]}; pr_.m[1] = f2{r.bj[2], r.bj[3]}; pr_.m[2] = f2{r.bj[4], r.bj[5]}; pr_.m[3] = f2{r.lj[0], r.lj[1]}; pr_.m[4] = f2{r.lj[2], 0.f};
    pr_.dinv = 1.0f / (d + QA_CFM);
    prow_store(rec, pr_);
}
// env-step persistents parked between substeps (act3 sp3 sd3 binert10) as five 16-byte records at QA_PRIV_STEP
QA_DEV void priv_park(float *priv, const float *act, const float *sp, const float *sd, const float *bi) {
    f4 *q = reinterpret_cast<f4 *>(priv + QA_PRIV_STEP);
    q[0] = f4{act[0], act[1], act[2], sp[0]}; q[1] = f4{sp[1], sp[2], sd[0], sd[1]}; q[2] = f4{sd[2], bi[0], bi[1], bi[2]};
    q[3] = f4{bi[3], bi[4], bi[5], bi[6]}; q[4] = f4{bi[7], bi[8], bi[9], 0.f};
}
QA_DEV void priv_unpark(const float *priv, float *act, float *sp, float *sd, float *bi) {
    const f4 *q = reinterpret_cast<const f4 *>(priv + QA_PRIV_STEP);
    const f4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    act[0] = a.x; act[1] = a.y; act[2] = a.z; sp[0] = a.w; sp[1] = b.x; sp[2] = b.y; sd[0] = b.z; sd[1] = b.w; sd[2] = c.x;
    bi[0] = c.y; bi[1] = c.z; bi[2] = c.w; bi[3] = d.x; bi[4] = d.y; bi[5] = d.z; bi[6] = d.w; bi[7] = e.x; bi[8] = e.y; bi[9] = e.z;
}

// Helper wavefronts (qa_env_step_kernel<..., HELP>): with one wavefront per CU three SIMDs of every CU idle, and the front half of a substep is
// three chains that meet only at the rows -- (composite inertias -> Schur complement), (bias forces), (contact candidates); all three need
// nothing but the kinematics of the state the substep starts from.  ROLE 1 (the env's own wavefront) publishes that state in LDS and keeps the
// first chain, ROLE 2 computes the bias forces and ROLE 3 the contact candidates from the same state on two other SIMDs and mail their results
// back: 19 + 9 + 10 floats per lane as 16-byte records, two workgroup barriers per substep.  ROLE 0 is the one-wavefront substep.  The same
// expressions on the same inputs: what ROLE 1 continues with is what ROLE 0 computed in place.
#define QA_MAIL_F4 13                    // 16-byte records per lane (odd: the 16 lanes of a b128 service group on different bank quads); 11 used
QA_DEV void mail_put_state(f4 *m, const EnvState &st) {
    m[0] = f4{st.pos.x, st.pos.y, st.pos.z, st.qx}; m[1] = f4{st.qy, st.qz, st.qw, st.vw.x}; m[2] = f4{st.vw.y, st.vw.z, st.ww.x, st.ww.y};
    m[3] = f4{st.ww.z, st.q[0], st.q[1], st.q[2]}; m[4] = f4{st.qd[0], st.qd[1], st.qd[2], 0.f};
}
QA_DEV void mail_get_state(const f4 *m, EnvState &st) {
    const f4 a = m[0], b = m[1], c = m[2], d = m[3], e = m[4];
    st.pos = v3(a.x, a.y, a.z); st.qx = a.w; st.qy = b.x; st.qz = b.y; st.qw = b.z; st.vw = v3(b.w, c.x, c.y); st.ww = v3(c.z, c.w, d.x);
    st.q[0] = d.y; st.q[1] = d.z; st.q[2] = d.w; st.qd[0] = e.x; st.qd[1] = e.y; st.qd[2] = e.z;
}

// With helper wavefronts the contact helper also builds the rows of the lane's non-foot contacts -- up to six rows, in the
// lane's LDS records where the sweeps read them anyway -- from the solve data (G, Binv, Linv in pairs: 63 floats as 16 records) the env's wavefront
// mails at the second barrier; a third barrier in front of the sweeps.
#define QA_MAIL_PS 11                    // first record of the solve data in a lane's mail
#undef QA_MAIL_F4
#define QA_MAIL_F4 29
QA_DEV void mail_put_solve(f4 *m, const PSolve &S) {
    const f2 *g = &S.G2[0][0], *b = &S.Bc[0][0];
    // 9 + 18 + 3 pairs = 30 pairs = 15 records, + L2 (3 floats)
    f2 q[30];
#pragma unroll
    for (int i = 0; i < 9; ++i) q[i] = g[i];
#pragma unroll
    for (int i = 0; i < 18; ++i) q[9 + i] = b[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[27 + i] = S.L01[i];
#pragma unroll
    for (int i = 0; i < 15; ++i) m[QA_MAIL_PS + i] = f4{q[2 * i].x, q[2 * i].y, q[2 * i + 1].x, q[2 * i + 1].y};
    m[QA_MAIL_PS + 15] = f4{S.L2[0], S.L2[1], S.L2[2], 0.f};
}
QA_DEV void mail_get_solve(const f4 *m, PSolve &S) {
    f2 q[30];
#pragma unroll
    for (int i = 0; i < 15; ++i) { const f4 v = m[QA_MAIL_PS + i]; q[2 * i] = f2{v.x, v.y}; q[2 * i + 1] = f2{v.z, v.w}; }
    f2 *g = &S.G2[0][0], *b = &S.Bc[0][0];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = q[i];
#pragma unroll
    for (int i = 0; i < 18; ++i) b[i] = q[9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) S.L01[i] = q[27 + i];
    const f4 l = m[QA_MAIL_PS + 15];
    S.L2[0] = l.x; S.L2[1] = l.y; S.L2[2] = l.z;
}

// idt (lp vp + l1 v1 + l2 v2), the world-frame force of a contact on sloped ground, with its multiply-adds SPELLED OUT: the product lp vp rounded, then
// one fused multiply-add per remaining term, in this order.  -ffp-contract=fast leaves the fusing of `idt * ((lam_n * n) + (lam_t1 * t1) + (lam_t2 * t2))`
// to the compiler, and it chooses per instantiation: read off the listings, every SCH = 0 kernel rounds lam_n n of the FOOT force and lam_t1 t1 of an
// extra slot's force, while the SCH = 1 kernels rounded lam_t1 t1 of the foot force -- the reported foot forces then differed in the last bit with no
// calf-hip pair anywhere near contact.  Only the SCH = 1 instantiations call this, with the terms in the SCH = 0 kernels' order: with the feature
// switched on and no pair in reach, every arena tensor stays bit-identical.
QA_DEV V3 sloped_contact_force(float lp, V3 vp, float l1, V3 v1, float l2, V3 v2, float idt) {
#pragma clang fp contract(off)
    const float x = __builtin_fmaf(l2, v2.x, __builtin_fmaf(l1, v1.x, lp * vp.x));
    const float y = __builtin_fmaf(l2, v2.y, __builtin_fmaf(l1, v1.y, lp * vp.y));
    const float z = __builtin_fmaf(l2, v2.z, __builtin_fmaf(l1, v1.z, lp * vp.z));
    return v3(idt * x, idt * y, idt * z);
}

template <bool PLANE, int ROLE = 0, int SCH = 0>
QA_DEV void phys_substep(EnvState &st, const float *tbl, const float *btbl, const float *binert, const float tau[3],
                         float mu, int leg, const PhysParams &P, ContactOut &co, float *priv, float fimp[3], const TerrainView &T, f4 *mail = nullptr) {
    static_assert(ROLE == 0 || PLANE, "helper wavefronts: plane kernels only (the height-field candidates carry six more values per contact)");
    const float dt = P.dt;
    M3 R = quat_to_mat(st.qx, st.qy, st.qz, st.qw);
    S6 V0 = s6(mulT(R, st.ww), mulT(R, st.vw));
    V3 gB = v3(R.m[6] * P.gz, R.m[7] * P.gz, R.m[8] * P.gz);

    QA_SUBSTAMP(0);
    // ---- leg kinematics in the base frame
    float s1, c1, s2, c2, s23, c23;
    __sincosf(st.q[0], &s1, &c1); __sincosf(st.q[1], &s2, &c2); __sincosf(st.q[1] + st.q[2], &s23, &c23);
    M3 Rl[3];
    Rl[0].m[0] = 1; Rl[0].m[1] = 0; Rl[0].m[2] = 0; Rl[0].m[3] = 0; Rl[0].m[4] = c1; Rl[0].m[5] = -s1; Rl[0].m[6] = 0; Rl[0].m[7] = s1; Rl[0].m[8] = c1;
    // R1 * Ry(t) = [[c,0,s],[s1 s, c1, -s1 c],[-c1 s, s1, c1 c]]
    Rl[1].m[0] = c2; Rl[1].m[1] = 0; Rl[1].m[2] = s2; Rl[1].m[3] = s1 * s2; Rl[1].m[4] = c1; Rl[1].m[5] = -s1 * c2; Rl[1].m[6] = -c1 * s2; Rl[1].m[7] = s1; Rl[1].m[8] = c1 * c2;
    Rl[2].m[0] = c23; Rl[2].m[1] = 0; Rl[2].m[2] = s23; Rl[2].m[3] = s1 * s23; Rl[2].m[4] = c1; Rl[2].m[5] = -s1 * c23; Rl[2].m[6] = -c1 * s23; Rl[2].m[7] = s1; Rl[2].m[8] = c1 * c23;
    V3 o[3], ax[3];
    o[0] = v3(tbl[T_HIP_ORG], tbl[T_HIP_ORG + 1], tbl[T_HIP_ORG + 2]);
    o[1] = o[0] + mul(Rl[0], v3(tbl[T_THIGH_ORG], tbl[T_THIGH_ORG + 1], tbl[T_THIGH_ORG + 2]));
    o[2] = o[1] + mul(Rl[1], v3(tbl[T_CALF_ORG], tbl[T_CALF_ORG + 1], tbl[T_CALF_ORG + 2]));
    ax[0] = v3(1, 0, 0); ax[1] = v3(0, c1, s1); ax[2] = ax[1];
    S6 S[3];
    RB link[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        S[k] = s6(ax[k], cross(o[k], ax[k]));
        link[k] = link_rb(tbl[T_MASS + k], v3(tbl[T_COM + 3 * k], tbl[T_COM + 3 * k + 1], tbl[T_COM + 3 * k + 2]),
                          tbl + T_INERTIA + 6 * k, Rl[k], o[k]);
    }
    QA_SUBSTAMP(1);
    RB base; base.m = binert[0]; base.h = v3(binert[1], binert[2], binert[3]);
    base.xx = binert[4]; base.yy = binert[5]; base.zz = binert[6]; base.xy = binert[7]; base.xz = binert[8]; base.yz = binert[9];
    float hl[3]; S6 f0;
    if (ROLE == 0 || ROLE == 2) {
    // ---- bias forces: Newton-Euler with zero joint acceleration, base acceleration = -gravity
    S6 A0 = s6(v3(0, 0, 0), v3(-gB.x, -gB.y, -gB.z));
    S6 fl[3];
    {
        S6 V = V0, A = A0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            S6 Sq = st.qd[k] * S[k];
            V = V + Sq;
            A = A + crm(V, Sq);
            fl[k] = apply(link[k], A) + crf(V, apply(link[k], V));
        }
    }
    fl[1] = fl[1] + fl[2]; fl[0] = fl[0] + fl[1];
    hl[0] = dot(S[0], fl[0]); hl[1] = dot(S[1], fl[1]); hl[2] = dot(S[2], fl[2]);
    f0 = apply(base, A0) + crf(V0, apply(base, V0)) + quad_sum(fl[0]);
    }
    if (ROLE == 2) {
        mail[5] = f4{hl[0], hl[1], hl[2], f0.a.x}; mail[6] = f4{f0.a.y, f0.a.z, f0.l.x, f0.l.y}; mail[7] = f4{f0.l.z, 0.f, 0.f, 0.f};
        __syncthreads();
        __syncthreads();                                     // (the contact helper's rows)
        return;
    }
    QA_SUBSTAMP(6);
    // ---- contact candidates: the foot sphere, and per extra slot (hip link + base share | thigh | calf) the point with the
    // smallest gap.  Only (gap, point code) are tracked; position, chain depth, body and terrain normal of a winner are rebuilt
    // when its rows are built, which only happens if some env of the wavefront has that slot in contact.
    V3 nB = v3(R.m[6], R.m[7], R.m[8]), t1B = v3(R.m[0], R.m[1], R.m[2]), t2B = v3(R.m[3], R.m[4], R.m[5]);   // plane: world z, x, y
    V3 foot_n = v3(0, 0, 1);                                 // world-frame contact normal (height field)
    float foot_gap = 0.f; V3 foot_p = v3(0, 0, 0);
    float foot_vs = 0.f, foot_ca = 0.f; int foot_ob = -1;    // articulated obstacle under the foot (surface velocity, joint lever, slot)
    float bgap[QA_EXTRA_GROUPS] = {1e30f, 1e30f, 1e30f};
    int bcode[QA_EXTRA_GROUPS] = {0, 0, 0};                  // 1..QA_LEG_PTS-1: leg point, 64 + c: base point
    auto leg_point = [&](int c, int k) {                     // base-frame position of leg point c (on link k)
        const float *pt = tbl + T_POINTS + 4 * c;
        // arithmetic blend over the links: any ?: between elements of Rl[] / o[] is folded by the compiler into a select of
        // INDICES, and a dynamically indexed register array lives in scratch
        const float w0 = k == 0 ? 1.f : 0.f, w1 = k == 1 ? 1.f : 0.f, w2 = k == 2 ? 1.f : 0.f;
        M3 Rs;
#pragma unroll
        for (int i = 0; i < 9; ++i) Rs.m[i] = fmaf(w0, Rl[0].m[i], fmaf(w1, Rl[1].m[i], w2 * Rl[2].m[i]));
        const V3 os = (w0 * o[0]) + (w1 * o[1]) + (w2 * o[2]);
        return mul(Rs, v3(pt[0], pt[1], pt[2])) + os;
    };
    if (ROLE != 1) {
    if (PLANE) {
        // On the plane only a candidate's world height matters: z_w = nB . (Rl_k pt + o_k) + z = (Rl_k^T nB) . pt + (nB . o_k + z),
        // i.e. 3 FMAs per point after 3 per-link vectors; the full base-frame position is built for winners only.
        V3 nk[3]; float hk[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { nk[k] = mulT(Rl[k], nB); hk[k] = dot(nB, o[k]) + st.pos.z; }
        {
            const float *pt = tbl + T_POINTS;
            foot_p = mul(Rl[2], v3(pt[0], pt[1], pt[2])) + o[2];
            foot_gap = dot(nB, foot_p) + st.pos.z - pt[3];
        }
#pragma unroll
        for (int c = 1; c < QA_LEG_PTS; ++c) {
            const int k = (c < 3 ? 0 : (c < 11 ? 1 : 2));
            const float *pt = tbl + T_POINTS + 4 * c;
            const float gap = dot(nk[k], v3(pt[0], pt[1], pt[2])) + hk[k] - pt[3];
            if (gap < bgap[k]) { bgap[k] = gap; bcode[k] = c; }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = leg + 4 * j;
            if (c < QA_BASE_PTS) {
                const float *pt = btbl + 4 * c;
                const float gap = dot(nB, v3(pt[0], pt[1], pt[2])) + st.pos.z - pt[3];
                if (gap < bgap[0]) { bgap[0] = gap; bcode[0] = 64 + c; }
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < QA_LEG_PTS; ++c) {
            const int k = (c == 0) ? 2 : (c < 3 ? 0 : (c < 11 ? 1 : 2));
            const float *pt = tbl + T_POINTS + 4 * c;
            V3 p = mul(Rl[k], v3(pt[0], pt[1], pt[2])) + o[k];
            float zw = dot(nB, p) + st.pos.z;
            V3 gn; float cvs, cca; int cob;
            float gap = contact_query(T, dot(t1B, p) + st.pos.x, dot(t2B, p) + st.pos.y, zw, pt[3], gn, cvs, cca, cob);      // distance to the terrain triangle's plane
            if (c == 0) { foot_gap = gap; foot_p = p; foot_n = gn; foot_vs = cvs; foot_ca = cca; foot_ob = cob; }
            else if (gap < bgap[k]) { bgap[k] = gap; bcode[k] = c; }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int c = leg + 4 * j;
            if (c < QA_BASE_PTS) {
                const float *pt = btbl + 4 * c;
                V3 p = v3(pt[0], pt[1], pt[2]);
                float zw = dot(nB, p) + st.pos.z;
                V3 gn; float gap = contact_query(T, dot(t1B, p) + st.pos.x, dot(t2B, p) + st.pos.y, zw, pt[3], gn);
                if (gap < bgap[0]) { bgap[0] = gap; bcode[0] = 64 + c; }
            }
        }
    }
    }
    // ---- which candidates make contact, compacted into the lane's slots 0..1 (group order)
    float sgap[QA_EXTRA_SLOTS]; int scode[QA_EXTRA_SLOTS], slink[QA_EXTRA_SLOTS];
    bool extra_on[QA_EXTRA_SLOTS], any_extra[QA_EXTRA_SLOTS];
    bool foot_on = false;
    if (ROLE != 1) {
        foot_on = foot_gap < P.contact_offset;
        bool on0 = bgap[0] < P.contact_offset, on1 = bgap[1] < P.contact_offset, on2 = bgap[2] < P.contact_offset;
        if (P.slots == 1) {        // cfg.contact_slots 1: only the lowest non-foot point of the leg (the round-1 model)
            const bool w1 = bgap[1] < bgap[0] && !(bgap[2] < bgap[1]), w2 = bgap[2] < bgap[0] && bgap[2] < bgap[1];
            on0 = on0 && !w1 && !w2; on1 = on1 && w1; on2 = on2 && w2;
        } else if (on0 && on1 && on2) {                      // three candidates, two slots: the largest gap waits
            const bool d0 = bgap[0] >= bgap[1] && bgap[0] >= bgap[2], d1 = !d0 && bgap[1] >= bgap[2];
            on0 = !d0; on1 = !d1; on2 = d0 || d1;
        }
        const int g0 = on0 ? 0 : (on1 ? 1 : (on2 ? 2 : -1));
        const int g1 = (g0 == 0) ? (on1 ? 1 : (on2 ? 2 : -1)) : ((g0 == 1 && on2) ? 2 : -1);
        // arithmetic blends, not ?: chains over the candidate arrays (see leg_point)
        const float a0 = g0 == 0 ? 1.f : 0.f, a1 = g0 == 1 ? 1.f : 0.f, a2 = g0 == 2 ? 1.f : 0.f, b1 = g1 == 1 ? 1.f : 0.f, b2 = g1 == 2 ? 1.f : 0.f;
        sgap[0] = g0 < 0 ? 1e30f : fmaf(a0, fminf(bgap[0], 1e20f), fmaf(a1, fminf(bgap[1], 1e20f), a2 * fminf(bgap[2], 1e20f)));
        sgap[1] = g1 < 0 ? 1e30f : fmaf(b1, fminf(bgap[1], 1e20f), b2 * fminf(bgap[2], 1e20f));
        scode[0] = (int)a0 * bcode[0] + (int)a1 * bcode[1] + (int)a2 * bcode[2];
        scode[1] = (int)b1 * bcode[1] + (int)b2 * bcode[2];
        slink[0] = g0; slink[1] = g1;
        extra_on[0] = g0 >= 0; extra_on[1] = g1 >= 0;
        any_extra[0] = __any(extra_on[0]); any_extra[1] = __any(extra_on[1]);
    }

    // ---- the rows of the lane's non-foot contacts (built by whoever holds the solve data PS: the one-wavefront substep and the env's wavefront
    // further down, or the contact helper right here, from the mail)
    PSolve PS;
    float re_lam[QA_EXTRA_SLOTS][3];
    float ex_ca[QA_EXTRA_SLOTS]; int ex_ob[QA_EXTRA_SLOTS];
    V3 ex_n[QA_EXTRA_SLOTS];                                // world-frame normals of the extra contacts (height field)
    int ex_body[QA_EXTRA_SLOTS];
    auto extra_rows = [&](int sl, bool build) {
        re_lam[sl][0] = re_lam[sl][1] = re_lam[sl][2] = 0.f; ex_n[sl] = v3(0, 0, 1); ex_body[sl] = -1; ex_ca[sl] = 0.f; ex_ob[sl] = -1;
        if (any_extra[sl]) {
            V3 p; int depth;
            const int code = scode[sl], link = max(slink[sl], 0);
            if (code >= 64) { const float *pt = btbl + 4 * (code - 64); p = v3(pt[0], pt[1], pt[2]); depth = 0; ex_body[sl] = (code - 64) < 8 ? 0 : ((code - 64) < 10 ? 1 : 2); }
            else { if (build) p = leg_point(code > 0 ? code : 1, link); depth = link + 1; ex_body[sl] = 3 + 4 * leg + link; }
            if (build) {
                PRow re[3];
                V3 en_b = nB, et1_b = t1B, et2_b = t2B;
                float ex_vs = 0.f;
                if (!PLANE) {
                    (void)contact_query(T, dot(t1B, p) + st.pos.x, dot(t2B, p) + st.pos.y, dot(nB, p) + st.pos.z, 0.f, ex_n[sl], ex_vs, ex_ca[sl], ex_ob[sl]);   // the winner's normal: floor or ceiling (both gaps carry the same -r, so the radius does not decide which is nearer)
                    V3 a, b; tangent_basis(ex_n[sl], a, b); en_b = mulT(R, ex_n[sl]); et1_b = mulT(R, a); et2_b = mulT(R, b);
                }
                pcontact_rows(re, p, depth, sgap[sl], ex_vs, o, ax, en_b, et1_b, et2_b, PS, P);
#pragma unroll
                for (int d = 0; d < 3; ++d) prow_store(priv + QA_PRIV_EXTRA + 60 * sl + 20 * d, re[d]);
            }
        }
    };
    if (ROLE == 3) {
        mail[8] = f4{foot_gap, foot_p.x, foot_p.y, foot_p.z};
        mail[9] = f4{sgap[0], sgap[1], __int_as_float(scode[0]), __int_as_float(scode[1])};
        mail[10] = f4{__int_as_float(slink[0]), __int_as_float(slink[1]), 0.f, 0.f};
        __syncthreads();
        mail_get_solve(mail, PS);                            // the env's wavefront wrote it in front of the barrier
#pragma unroll
        for (int sl = 0; sl < QA_EXTRA_SLOTS; ++sl) extra_rows(sl, true);
        __syncthreads();                                     // the rows are in the lane's LDS records: the sweeps may start
        return;
    }
    QA_SUBSTAMP(2);
    // ---- composite inertias, mass-matrix blocks
    RB Ic2 = link[2], Ic1 = link[1] + Ic2, Ic0 = link[0] + Ic1;
    S6 F[3] = {apply(Ic0, S[0]), apply(Ic1, S[1]), apply(Ic2, S[2])};
    float L00 = dot(S[0], F[0]), L01 = dot(S[0], F[1]), L02 = dot(S[0], F[2]);
    float L11 = dot(S[1], F[1]), L12 = dot(S[1], F[2]), L22 = dot(S[2], F[2]);
    RB tot = base + quad_sum(Ic0);

    QA_SUBSTAMP(3);
    // ---- leg elimination: Linv (packed 00 01 02 11 12 22), G = -Linv F^T (3x6 row-major)
    float Linv[6];
    {
        float cA = L11 * L22 - L12 * L12, cB = L02 * L12 - L01 * L22, cC = L01 * L12 - L02 * L11;
        float cD = L00 * L22 - L02 * L02, cE = L01 * L02 - L00 * L12, cF = L00 * L11 - L01 * L01;
        float idet = 1.0f / (L00 * cA + L01 * cB + L02 * cC);
        Linv[0] = cA * idet; Linv[1] = cB * idet; Linv[2] = cC * idet; Linv[3] = cD * idet; Linv[4] = cE * idet; Linv[5] = cF * idet;
    }
    float Fm[3][6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Fm[k][0] = F[k].a.x; Fm[k][1] = F[k].a.y; Fm[k][2] = F[k].a.z; Fm[k][3] = F[k].l.x; Fm[k][4] = F[k].l.y; Fm[k][5] = F[k].l.z; }
    float G[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        G[0 * 6 + i] = -(Linv[0] * Fm[0][i] + Linv[1] * Fm[1][i] + Linv[2] * Fm[2][i]);
        G[1 * 6 + i] = -(Linv[1] * Fm[0][i] + Linv[3] * Fm[1][i] + Linv[4] * Fm[2][i]);
        G[2 * 6 + i] = -(Linv[2] * Fm[0][i] + Linv[4] * Fm[1][i] + Linv[5] * Fm[2][i]);
    }
    // Schur complement of the base: Mbb + sum_legs F G   (packed symmetric 6x6)
    float Bm[21];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
            Bm[SIDX(i, j)] = quad_sum(Fm[0][i] * G[0 * 6 + j] + Fm[1][i] * G[1 * 6 + j] + Fm[2][i] * G[2 * 6 + j]);
    Bm[SIDX(0, 0)] += tot.xx; Bm[SIDX(1, 1)] += tot.yy; Bm[SIDX(2, 2)] += tot.zz;
    Bm[SIDX(1, 0)] += tot.xy; Bm[SIDX(2, 0)] += tot.xz; Bm[SIDX(2, 1)] += tot.yz;
    Bm[SIDX(3, 3)] += tot.m; Bm[SIDX(4, 4)] += tot.m; Bm[SIDX(5, 5)] += tot.m;
    // lower-left block M[3+j][i] = hx[i][j], hx = [h]x
    Bm[SIDX(3, 1)] += tot.h.z; Bm[SIDX(3, 2)] += -tot.h.y;
    Bm[SIDX(4, 0)] += -tot.h.z; Bm[SIDX(4, 2)] += tot.h.x;
    Bm[SIDX(5, 0)] += tot.h.y; Bm[SIDX(5, 1)] += -tot.h.x;
    float Binv[21];
    spd6_inverse(Bm, Binv);
    psolve_make(PS, G, Linv, Binv);
    if (ROLE == 1) mail_put_solve(mail, PS);
    if (ROLE == 1) {
        __syncthreads();                                     // the helpers' results of THIS substep are in the mail
        const f4 a = mail[5], b = mail[6], c = mail[7], d = mail[8], e = mail[9], g = mail[10];
        hl[0] = a.x; hl[1] = a.y; hl[2] = a.z; f0 = s6(v3(a.w, b.x, b.y), v3(b.z, b.w, c.x));
        foot_gap = d.x; foot_p = v3(d.y, d.z, d.w);
        sgap[0] = e.x; sgap[1] = e.y; scode[0] = __float_as_int(e.z); scode[1] = __float_as_int(e.w);
        slink[0] = __float_as_int(g.x); slink[1] = __float_as_int(g.y);
        foot_on = foot_gap < P.contact_offset;
        extra_on[0] = slink[0] >= 0; extra_on[1] = slink[1] >= 0;
        any_extra[0] = __any(extra_on[0]); any_extra[1] = __any(extra_on[1]);
    }

    QA_SUBSTAMP(5);
    // ---- unconstrained velocity
    float rl[3] = {tau[0] - hl[0], tau[1] - hl[1], tau[2] - hl[2]};
    float rb[6] = {-f0.a.x, -f0.a.y, -f0.a.z, -f0.l.x, -f0.l.y, -f0.l.z};
#pragma unroll
    for (int i = 0; i < 6; ++i) rb[i] += quad_sum(G[0 * 6 + i] * rl[0] + G[1 * 6 + i] * rl[1] + G[2 * 6 + i] * rl[2]);
    float ab[6];
    sym6_mul(Binv, rb, ab);
    V3 wxv = cross(V0.a, V0.l);
    float ub[6] = {V0.a.x + dt * ab[0], V0.a.y + dt * ab[1], V0.a.z + dt * ab[2],
                   V0.l.x + dt * (ab[3] + wxv.x), V0.l.y + dt * (ab[4] + wxv.y), V0.l.z + dt * (ab[5] + wxv.z)};
    float w[3];   // w = u_leg* - G ub*  with u_leg* = qd + dt (Linv r + G ab)  =>  w = qd + dt Linv r + G (dt ab - ub*)... keep it explicit:
    {
        float lr0 = Linv[0] * rl[0] + Linv[1] * rl[1] + Linv[2] * rl[2];
        float lr1 = Linv[1] * rl[0] + Linv[3] * rl[1] + Linv[4] * rl[2];
        float lr2 = Linv[2] * rl[0] + Linv[4] * rl[1] + Linv[5] * rl[2];
        float lr[3] = {lr0, lr1, lr2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float gab = 0.f, gub = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) { gab = fmaf(G[k * 6 + i], ab[i], gab); gub = fmaf(G[k * 6 + i], ub[i], gub); }
            float ul = st.qd[k] + dt * (lr[k] + gab);
            w[k] = ul - gub;
        }
    }

    QA_SUBSTAMP(7);
    // ---- rows, packed (see PRow): foot rows in registers; the extra slots' and the self-collision rows in the lane's LDS records, built only
    // when some env of the wavefront needs them
    PRow rf[3];
    V3 fn_b = nB, ft1_b = t1B, ft2_b = t2B, ft1_w = v3(1, 0, 0), ft2_w = v3(0, 1, 0);
    if (!PLANE) { tangent_basis(foot_n, ft1_w, ft2_w); fn_b = mulT(R, foot_n); ft1_b = mulT(R, ft1_w); ft2_b = mulT(R, ft2_w); }
    pcontact_rows(rf, foot_p, 3, foot_gap, foot_vs, o, ax, fn_b, ft1_b, ft2_b, PS, P);
    // Per-LANE activity is carried by the rows' data, not by branches: a row whose contact is open gets a bias no velocity overcomes
    // (residual > 0 => lam stays 0 => x + m 0 = x exactly), so the sweeps below branch on wave-uniform votes only -- a lane-divergent `if`
    // costs ~8 scalar instructions of exec-mask bookkeeping per block and saves nothing (the idle lanes' slots are issued anyway).
    rf[0].j[4].y = foot_on ? rf[0].j[4].y : QA_OPEN_BIAS;
#pragma unroll
    for (int sl = 0; sl < QA_EXTRA_SLOTS; ++sl) extra_rows(sl, ROLE != 1);      // with helpers: the contact helper is building them meanwhile
    // ---- self-collision rows: partner 0 = lane ^ 1 (left / right), partner 1 = lane ^ 2 (front / rear).  Both lanes of a pair evaluate the
    // SAME expressions on the same (canonically ordered) segments, so they agree bit for bit on gap, normal and effective mass.  This path is
    // rare (4e-6 of the env-steps of a training run) and stays in scalar arithmetic; only its LDS record is the packed one.
    bool sc_on[2] = {false, false}, any_sc[2] = {false, false}, sc_low[2] = {false, false};
    float sc_lam[2] = {0.f, 0.f};
    V3 sc_nw[2];
    if (P.self_collision) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const V3 a0 = o[2], a1 = foot_p;
            V3 b0, b1;
            if (pr == 0) { b0 = v3(dpp_f<0xB1>(a0.x), dpp_f<0xB1>(a0.y), dpp_f<0xB1>(a0.z)); b1 = v3(dpp_f<0xB1>(a1.x), dpp_f<0xB1>(a1.y), dpp_f<0xB1>(a1.z)); }
            else { b0 = v3(dpp_f<0x4E>(a0.x), dpp_f<0x4E>(a0.y), dpp_f<0x4E>(a0.z)); b1 = v3(dpp_f<0x4E>(a1.x), dpp_f<0x4E>(a1.y), dpp_f<0x4E>(a1.z)); }
            const bool low = pr == 0 ? ((leg & 1) == 0) : ((leg & 2) == 0);          // this lane holds the pair's first capsule
            const V3 A0 = low ? a0 : b0, A1 = low ? a1 : b1, B0 = low ? b0 : a0, B1 = low ? b1 : a1;
            float sa, tb; segment_closest(A0, A1, B0, B1, sa, tb);
            const V3 pA = A0 + sa * (A1 - A0), pB = B0 + tb * (B1 - B0), dv = pA - pB;
            const float dist = sqrtf(dot(dv, dv));
            const V3 nrm = dist > 1e-6f ? (1.0f / dist) * dv : v3(0.f, 1.f, 0.f);
            const float gap = dist - (QA_CALF_RADIUS + sa * (QA_FOOT_RADIUS - QA_CALF_RADIUS)) - (QA_CALF_RADIUS + tb * (QA_FOOT_RADIUS - QA_CALF_RADIUS));
            sc_on[pr] = gap < P.contact_offset; sc_low[pr] = low;
            any_sc[pr] = __any(sc_on[pr]);
            sc_nw[pr] = low ? nrm : v3(-nrm.x, -nrm.y, -nrm.z);          // base frame: direction of the force on THIS leg
            if (any_sc[pr]) {
                Row r;
                const V3 pm = low ? pA : pB;
#pragma unroll
                for (int k = 0; k < 3; ++k) r.jl[k] = dot(sc_nw[pr], cross(ax[k], pm - o[k]));
                float h[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) h[i] = G[0 * 6 + i] * r.jl[0] + G[1 * 6 + i] * r.jl[1] + G[2 * 6 + i] * r.jl[2];
#pragma unroll
                for (int i = 0; i < 6; ++i) r.jh[i] = h[i] + (pr == 0 ? dpp_f<0xB1>(h[i]) : dpp_f<0x4E>(h[i]));
                sym6_mul(Binv, r.jh, r.bj);
                r.lj[0] = Linv[0] * r.jl[0] + Linv[1] * r.jl[1] + Linv[2] * r.jl[2];
                r.lj[1] = Linv[1] * r.jl[0] + Linv[3] * r.jl[1] + Linv[4] * r.jl[2];
                r.lj[2] = Linv[2] * r.jl[0] + Linv[4] * r.jl[1] + Linv[5] * r.jl[2];
                const float dleg = r.jl[0] * r.lj[0] + r.jl[1] * r.lj[1] + r.jl[2] * r.lj[2];
                float d = dleg + (pr == 0 ? dpp_f<0xB1>(dleg) : dpp_f<0x4E>(dleg));
#pragma unroll
                for (int i = 0; i < 6; ++i) d = fmaf(r.jh[i], r.bj[i], d);
                const float g = gap / dt;
                PRow pr_;
                pr_.j[0] = f2{r.jh[0], r.jh[1]}; pr_.j[1] = f2{r.jh[2], r.jh[3]}; pr_.j[2] = f2{r.jh[4], r.jh[5]}; pr_.j[3] = f2{r.jl[0], r.jl[1]};
                pr_.j[4] = f2{r.jl[2], gap >= 0.f ? g : fmaxf(g, -P.max_depen)};
                pr_.m[0] = f2{r.bj[0], r.bj[1]}; pr_.m[1] = f2{r.bj[2], r.bj[3]}; pr_.m[2] = f2{r.bj[4], r.bj[5]}; pr_.m[3] = f2{r.lj[0], r.lj[1]}; pr_.m[4] = f2{r.lj[2], 0.f};
                pr_.dinv = 1.0f / (d + QA_CFM);
                prow_store(priv + QA_PRIV_SELF + 20 * pr, pr_);
            }
        }
    }
    // ---- calf against the neighbouring hip (SCH): the pair is (front leg, rear leg of the same side) = lane ^ 2; the front lane holds the calf,
    // the rear lane the hip.  Both evaluate qa_sc_calf_hip on the SAME four points (calf first), so they agree bit for bit on gap and normal;
    // the row is built and swept exactly like a front / rear calf-calf row.  Rare: scalar arithmetic, the row in the lane's LDS record.
    bool sh_on = false, any_sh = false;
    const bool sh_calf = (leg & 2) == 0;
    float sh_lam = 0.f;
    V3 sh_nw = v3(0.f, 0.f, 0.f);
    if constexpr (SCH != 0) {
        const float org[3] = {o[0].x, o[0].y, o[0].z};
        float h0[3], h1[3];
        qa_sc_hip_segment(org, c1, s1, (leg & 1) ? -1.f : 1.f, h0, h1);
        // a lane sends what its side of the pair contributes and receives the other side's: 6 quad_perm moves
        const float snd[6] = {sh_calf ? o[2].x : h0[0], sh_calf ? o[2].y : h0[1], sh_calf ? o[2].z : h0[2],
                              sh_calf ? foot_p.x : h1[0], sh_calf ? foot_p.y : h1[1], sh_calf ? foot_p.z : h1[2]};
        float cs[6], hs[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { const float rcv = dpp_f<0x4E>(snd[i]); cs[i] = sh_calf ? snd[i] : rcv; hs[i] = sh_calf ? rcv : snd[i]; }
        qa_sc_contact ct;
        qa_sc_calf_hip(cs, cs + 3, hs, hs + 3, &ct);
        sh_on = ct.gap < P.contact_offset;
        any_sh = __any(sh_on);
        const float sg = sh_calf ? 1.f : -1.f;
        sh_nw = v3(sg * ct.n[0], sg * ct.n[1], sg * ct.n[2]);       // base frame: direction of the force on THIS leg's body
        co.sh_dir = mul(R, sh_nw);
        if (any_sh) {
            Row r;
            const V3 pm = sh_calf ? v3(ct.pc[0], ct.pc[1], ct.pc[2]) : v3(ct.ph[0], ct.ph[1], ct.ph[2]);
            r.jl[0] = dot(sh_nw, cross(ax[0], pm - o[0]));
            // the hip cylinder rides on the hip link: joints 1 and 2 of its leg do not move it
            r.jl[1] = sh_calf ? dot(sh_nw, cross(ax[1], pm - o[1])) : 0.f;
            r.jl[2] = sh_calf ? dot(sh_nw, cross(ax[2], pm - o[2])) : 0.f;
            float h[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) h[i] = G[0 * 6 + i] * r.jl[0] + G[1 * 6 + i] * r.jl[1] + G[2 * 6 + i] * r.jl[2];
#pragma unroll
            for (int i = 0; i < 6; ++i) r.jh[i] = h[i] + dpp_f<0x4E>(h[i]);
            sym6_mul(Binv, r.jh, r.bj);
            r.lj[0] = Linv[0] * r.jl[0] + Linv[1] * r.jl[1] + Linv[2] * r.jl[2];
            r.lj[1] = Linv[1] * r.jl[0] + Linv[3] * r.jl[1] + Linv[4] * r.jl[2];
            r.lj[2] = Linv[2] * r.jl[0] + Linv[4] * r.jl[1] + Linv[5] * r.jl[2];
            const float dleg = r.jl[0] * r.lj[0] + r.jl[1] * r.lj[1] + r.jl[2] * r.lj[2];
            float d = dleg + dpp_f<0x4E>(dleg);
#pragma unroll
            for (int i = 0; i < 6; ++i) d = fmaf(r.jh[i], r.bj[i], d);
            const float g = ct.gap / dt;
            PRow pr_;
            pr_.j[0] = f2{r.jh[0], r.jh[1]}; pr_.j[1] = f2{r.jh[2], r.jh[3]}; pr_.j[2] = f2{r.jh[4], r.jh[5]}; pr_.j[3] = f2{r.jl[0], r.jl[1]};
            pr_.j[4] = f2{r.jl[2], ct.gap >= 0.f ? g : fmaxf(g, -P.max_depen)};
            pr_.m[0] = f2{r.bj[0], r.bj[1]}; pr_.m[1] = f2{r.bj[2], r.bj[3]}; pr_.m[2] = f2{r.bj[4], r.bj[5]}; pr_.m[3] = f2{r.lj[0], r.lj[1]}; pr_.m[4] = f2{r.lj[2], 0.f};
            pr_.dinv = 1.0f / (d + QA_CFM);
            prow_store(priv + QA_PRIV_HIPS, pr_);
        }
    }
    // ---- calf against the front / rear neighbour's thigh (SCH = 2): the same pair, lane ^ 2, with two rows -- row 0 the front leg's calf on the rear
    // leg's thigh, row 1 the rear leg's calf on the front leg's thigh.  Each lane sends its calf and its thigh segment and both evaluate
    // qa_sc_calf_thigh on the same role-ordered points (calf first), so they agree bit for bit.  Chain depth 3 on the calf's side, 2 on the thigh's
    // (the calf joint does not move the thigh).  One vote for both rows: rarer than the calf-hip row's build is cheap.
    bool st_on[2] = {false, false}, any_st = false;
    float st_lam[2] = {0.f, 0.f};
    if constexpr (SCH >= 2) {
        const float torg[3] = {o[1].x, o[1].y, o[1].z}, knee[3] = {o[2].x, o[2].y, o[2].z};
        float th0[3], th1[3];
        qa_sc_thigh_segment(torg, knee, th0, th1);
        const float own[12] = {o[2].x, o[2].y, o[2].z, foot_p.x, foot_p.y, foot_p.z, th0[0], th0[1], th0[2], th1[0], th1[1], th1[2]};
        float oth[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) oth[i] = dpp_f<0x4E>(own[i]);
        qa_sc_contact ct[2];
        V3 st_nw[2];
        bool st_calf[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            st_calf[r] = sh_calf == (r == 0);                 // this lane holds the row's calf
            float cs[6], ts[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) { cs[i] = st_calf[r] ? own[i] : oth[i]; ts[i] = st_calf[r] ? oth[6 + i] : own[6 + i]; }
            qa_sc_calf_thigh(cs, cs + 3, ts, ts + 3, &ct[r]);
            st_on[r] = ct[r].gap < P.contact_offset;
            const float sg = st_calf[r] ? 1.f : -1.f;
            st_nw[r] = v3(sg * ct[r].n[0], sg * ct[r].n[1], sg * ct[r].n[2]);       // base frame: direction of the force on THIS leg's body
            co.st_dir[r] = mul(R, st_nw[r]);
        }
        any_st = __any(st_on[0] || st_on[1]);
        if (any_st) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const V3 pm = st_calf[r] ? v3(ct[r].pc[0], ct[r].pc[1], ct[r].pc[2]) : v3(ct[r].ph[0], ct[r].ph[1], ct[r].ph[2]);
                const float jl[3] = {dot(st_nw[r], cross(ax[0], pm - o[0])), dot(st_nw[r], cross(ax[1], pm - o[1])),
                                     st_calf[r] ? dot(st_nw[r], cross(ax[2], pm - o[2])) : 0.f};
                pair_row_store(priv + QA_PRIV_THIGHS + 20 * r, jl, G, Linv, Binv, ct[r].gap, dt, P.max_depen);
            }
        }
    }
    // joint limits: at most one stop per joint can be within the margin.  jl = sgn e_k  =>  jh = sgn G[k,:], lj = sgn Linv[:,k]
    float lim_sgn[3], lim_bias[3], lim_lam[3], lim_dinv[3];   // registers: these rows run in most waves
    f2 lim_m[3][3];
    bool lim_on[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float glo = st.q[k] - tbl[T_LOWER + k], ghi = tbl[T_UPPER + k] - st.q[k];
        bool lo = glo < QA_LIMIT_MARGIN, hi = !lo && (ghi < QA_LIMIT_MARGIN);
        lim_on[k] = lo || hi;
        lim_sgn[k] = lo ? 1.f : -1.f;
        float gap = lo ? glo : ghi, g = gap / dt;
        lim_bias[k] = lim_on[k] ? (gap >= 0.f ? g : fmaxf(g, -QA_LIMIT_DEPEN)) : QA_OPEN_BIAS;
        lim_lam[k] = 0.f;
    }
    const bool any_limk[3] = {(bool)__any(lim_on[0]), (bool)__any(lim_on[1]), (bool)__any(lim_on[2])};
    const bool any_lim = any_limk[0] || any_limk[1] || any_limk[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (any_limk[k]) {
            f2 jh[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) jh[q] = f2s(lim_sgn[k]) * PS.G2[k][q];
            pbinv_mul(PS, jh, lim_m[k]);
            const float lkk = (k == 0) ? Linv[0] : (k == 1 ? Linv[3] : Linv[5]);
            const f2 dd = pfma(jh[2], lim_m[k][2], pfma(jh[1], lim_m[k][1], jh[0] * lim_m[k][0]));
            lim_dinv[k] = 1.0f / (lkk + hsum(dd) + QA_CFM);
        }
    }

    QA_SUBSTAMP(8);
    // ---- the sweeps' state: x = (ub | w, 1).  Warm start: the foot rows start from the previous substep's impulses, applied to x first
    // (the base part summed over the quad, the leg part local)
    f2 x[5] = {f2{ub[0], ub[1]}, f2{ub[2], ub[3]}, f2{ub[4], ub[5]}, f2{w[0], w[1]}, f2{w[2], 1.0f}};
    {
        f2 dx[5] = {f2s(0.f), f2s(0.f), f2s(0.f), x[3], x[4]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float l0 = foot_on ? fimp[d] : 0.f;
            rf[d].lam = l0;
#pragma unroll
            for (int i = 0; i < 5; ++i) dx[i] = pfma(rf[d].m[i], f2s(l0), dx[i]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) x[q] += f2{quad_sum(dx[q].x), quad_sum(dx[q].y)};
        x[3] = dx[3]; x[4] = dx[4];
    }
    if (ROLE == 1) __syncthreads();         // the contact helper's rows of this substep are in the lane's LDS records
    QA_SUBSTAMP(4);
    // ---- projected Gauss-Seidel with a two-colour ordering over the legs: the diagonal pairs {FL, RR} and {FR, RL} are
    // updated from the same base velocity and their base-velocity changes are summed; colours follow each other Gauss-Seidel fashion.  Every
    // lane runs its own rows in both passes and only the lanes of the active colour commit (the lanes of a quad run in lockstep: the idle
    // colour's instructions are issued anyway).  Commit: the base takes d[a] + d[b] of the two active lanes a, b through two quad_perm
    // broadcasts per component, in the same order on all four lanes (they must keep bit-identical copies of ub).
    const bool any_foot = __any(foot_on);
    const bool colour_a = ((leg + 1) & 2) == 0;          // legs 0 and 3, without a short-circuit
    for (int it = 0; it < P.iters; ++it) {
#pragma unroll
        for (int colour = 0; colour < 2; ++colour) {
            const bool mine = (colour == 0) == colour_a;
            f2 x2[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) x2[i] = x[i];
            if (any_foot) {
                const float l0 = rf[0].lam, l1 = rf[1].lam, l2 = rf[2].lam;
                pcontact_update(rf, x2, mu);
                rf[0].lam = mine ? rf[0].lam : l0; rf[1].lam = mine ? rf[1].lam : l1; rf[2].lam = mine ? rf[2].lam : l2;
            }
#pragma unroll
            for (int sl = 0; sl < QA_EXTRA_SLOTS; ++sl) {
                if (any_extra[sl]) {          // a lane without this slot's contact holds rows with gap 1e30: they leave x alone
                    // Most non-foot candidates inside the contact offset are NOT pressing (a calf 5 mm above the ground): the normal row's
                    // impulse stays 0 and the whole update is x + m 0.  One normal-row residual (5 of the 15 LDS reads, 10 of the ~50
                    // instructions) decides it for the wavefront; skipping is exact -- what is skipped would have changed nothing.
                    PRow t[3];
                    prow_load(priv + QA_PRIV_EXTRA + 60 * sl, t[0]);
                    t[0].lam = re_lam[sl][0];
                    const float lam_try = fmaxf(fmaf(-prow_residual(t[0], x2), t[0].dinv, t[0].lam), 0.f);
                    const bool live = lam_try != 0.f || t[0].lam != 0.f || re_lam[sl][1] != 0.f || re_lam[sl][2] != 0.f;
                    if (__any(live)) {
                        prow_load(priv + QA_PRIV_EXTRA + 60 * sl + 20, t[1]); prow_load(priv + QA_PRIV_EXTRA + 60 * sl + 40, t[2]);
                        t[1].lam = re_lam[sl][1]; t[2].lam = re_lam[sl][2];
                        pcontact_update(t, x2, mu);
                        re_lam[sl][0] = mine ? t[0].lam : re_lam[sl][0]; re_lam[sl][1] = mine ? t[1].lam : re_lam[sl][1]; re_lam[sl][2] = mine ? t[2].lam : re_lam[sl][2];
                    }
                }
            }
            {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (any_limk[k]) {
                        // residual = bias + sgn * u_k,   u_k = w_k + G[k,:] ub
                        const f2 gu = pfma(PS.G2[k][2], x2[2], pfma(PS.G2[k][1], x2[1], PS.G2[k][0] * x2[0]));
                        const float wk = k == 0 ? x2[3].x : (k == 1 ? x2[3].y : x2[4].x);
                        const float uk = hsum(gu) + wk;
                        const float res = fmaf(lim_sgn[k], uk, lim_bias[k]);
                        const float lam = fmaxf(fmaf(-res, lim_dinv[k], lim_lam[k]), 0.f);
                        const float dl = lam - lim_lam[k];
                        if (__any(dl != 0.f)) {          // a joint inside the margin but not at its stop: nothing to apply (exact skip, as above)
                            lim_lam[k] = mine ? lam : lim_lam[k];
#pragma unroll
                            for (int q = 0; q < 3; ++q) x2[q] = pfma(lim_m[k][q], f2s(dl), x2[q]);
                            const float sd = lim_sgn[k] * dl;
                            x2[3] = pfma(PS.L01[k], f2s(sd), x2[3]);
                            x2[4].x = fmaf(PS.L2[k], sd, x2[4].x);
                        }
                    }
                }
            }
            // commit: lanes of the active colour keep their w; the base takes the SUM of the two active lanes' velocity changes.
            // Selects, not `if (mine) { x[3] = x2[3]; x[4].x = x2[4].x; }`: hipcc 7.2 (-O1 and -O3 alike) turns that element-wise conditional
            // copy of a 2-vector under `leg == 0 || leg == 3` into two nested exec regions and restores x[4].x for leg 0 as well -- the calf
            // joint of the front-left leg then never receives its contact impulse (found by tools/ab_lockstep.py: every first touchdown
            // that diverged from the scalar build was an FL foot; profiles/r5_packed_sweeps_debug.txt)
            x[3].x = mine ? x2[3].x : x[3].x; x[3].y = mine ? x2[3].y : x[3].y; x[4].x = mine ? x2[4].x : x[4].x;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const f2 d = x2[q] - x[q];
                if (colour == 0) {
                    x[q].x = (x[q].x + dpp_f<0x00>(d.x)) + dpp_f<0xFF>(d.x);      // lanes 0 and 3 (FL, RR)
                    x[q].y = (x[q].y + dpp_f<0x00>(d.y)) + dpp_f<0xFF>(d.y);
                } else {
                    x[q].x = (x[q].x + dpp_f<0x55>(d.x)) + dpp_f<0xAA>(d.x);      // lanes 1 and 2 (FR, RL)
                    x[q].y = (x[q].y + dpp_f<0x55>(d.y)) + dpp_f<0xAA>(d.y);
                }
            }
        }
        // self-collision pairs: the two left/right pairs from the same base velocity (their base-velocity changes summed, one lane of a
        // pair reporting it), then the two front/rear pairs
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            if (any_sc[pr]) {
                // every lane of the wavefront runs the row it stored (built under the same vote); a lane whose pair is apart takes dl = 0 -- no
                // lane-divergent region around vector-element writes (see the commit above)
                PRow r; prow_load(priv + QA_PRIV_SELF + 20 * pr, r);
                const float tl = r.j[3].x * x[3].x + r.j[3].y * x[3].y + r.j[4].x * x[4].x;
                // own + partner term FIRST: the sum is commutative, so both lanes of the pair hold identical bits before the (identical) bias
                // and base chain are added -- (bias + own) + partner rounds differently on the two sides and lets their lam drift apart
                const float tls = tl + (pr == 0 ? dpp_f<0xB1>(tl) : dpp_f<0x4E>(tl));
                float res = r.j[4].y + tls;
                res = fmaf(r.j[0].x, x[0].x, res); res = fmaf(r.j[0].y, x[0].y, res); res = fmaf(r.j[1].x, x[1].x, res);
                res = fmaf(r.j[1].y, x[1].y, res); res = fmaf(r.j[2].x, x[2].x, res); res = fmaf(r.j[2].y, x[2].y, res);
                const float lam = sc_on[pr] ? fmaxf(sc_lam[pr] - res * r.dinv, 0.f) : sc_lam[pr], dl = lam - sc_lam[pr];
                sc_lam[pr] = lam;
                x[3] = pfma(r.m[3], f2s(dl), x[3]);
                x[4].x = fmaf(r.m[4].x, dl, x[4].x);
                const float dlb = sc_low[pr] ? dl : 0.f;
                const f2 db0 = r.m[0] * f2s(dlb), db1 = r.m[1] * f2s(dlb), db2 = r.m[2] * f2s(dlb);
                x[0] += f2{quad_sum(db0.x), quad_sum(db0.y)}; x[1] += f2{quad_sum(db1.x), quad_sum(db1.y)}; x[2] += f2{quad_sum(db2.x), quad_sum(db2.y)};
            }
        }
        // calf-hip pairs (SCH): the two front / rear pairs from the same base velocity, the front lane of a pair reporting its base-velocity change;
        // the same wave-uniform vote, the same own + partner ordering and the same dl = 0 for a lane whose pair is apart as above
        if constexpr (SCH != 0) {
            if (any_sh) {
                PRow r; prow_load(priv + QA_PRIV_HIPS, r);
                const float tl = r.j[3].x * x[3].x + r.j[3].y * x[3].y + r.j[4].x * x[4].x;
                const float tls = tl + dpp_f<0x4E>(tl);
                float res = r.j[4].y + tls;
                res = fmaf(r.j[0].x, x[0].x, res); res = fmaf(r.j[0].y, x[0].y, res); res = fmaf(r.j[1].x, x[1].x, res);
                res = fmaf(r.j[1].y, x[1].y, res); res = fmaf(r.j[2].x, x[2].x, res); res = fmaf(r.j[2].y, x[2].y, res);
                const float lam = sh_on ? fmaxf(sh_lam - res * r.dinv, 0.f) : sh_lam, dl = lam - sh_lam;
                sh_lam = lam;
                x[3] = pfma(r.m[3], f2s(dl), x[3]);
                x[4].x = fmaf(r.m[4].x, dl, x[4].x);
                const float dlb = sh_calf ? dl : 0.f;
                const f2 db0 = r.m[0] * f2s(dlb), db1 = r.m[1] * f2s(dlb), db2 = r.m[2] * f2s(dlb);
                x[0] += f2{quad_sum(db0.x), quad_sum(db0.y)}; x[1] += f2{quad_sum(db1.x), quad_sum(db1.y)}; x[2] += f2{quad_sum(db2.x), quad_sum(db2.y)};
            }
        }
        // calf-thigh pairs (SCH = 2): a fourth pair phase, its two rows one after the other, each with the vote, the ordering and the dl = 0 of the
        // calf-hip phase; the front lane of a pair reports the base-velocity change of both rows
        if constexpr (SCH >= 2) {
            if (any_st) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    PRow r; prow_load(priv + QA_PRIV_THIGHS + 20 * k, r);
                    const float tl = r.j[3].x * x[3].x + r.j[3].y * x[3].y + r.j[4].x * x[4].x;
                    const float tls = tl + dpp_f<0x4E>(tl);
                    float res = r.j[4].y + tls;
                    res = fmaf(r.j[0].x, x[0].x, res); res = fmaf(r.j[0].y, x[0].y, res); res = fmaf(r.j[1].x, x[1].x, res);
                    res = fmaf(r.j[1].y, x[1].y, res); res = fmaf(r.j[2].x, x[2].x, res); res = fmaf(r.j[2].y, x[2].y, res);
                    const float lam = st_on[k] ? fmaxf(st_lam[k] - res * r.dinv, 0.f) : st_lam[k], dl = lam - st_lam[k];
                    st_lam[k] = lam;
                    x[3] = pfma(r.m[3], f2s(dl), x[3]);
                    x[4].x = fmaf(r.m[4].x, dl, x[4].x);
                    const float dlb = sh_calf ? dl : 0.f;
                    const f2 db0 = r.m[0] * f2s(dlb), db1 = r.m[1] * f2s(dlb), db2 = r.m[2] * f2s(dlb);
                    x[0] += f2{quad_sum(db0.x), quad_sum(db0.y)}; x[1] += f2{quad_sum(db1.x), quad_sum(db1.y)}; x[2] += f2{quad_sum(db2.x), quad_sum(db2.y)};
                }
            }
        }
    }
    ub[0] = x[0].x; ub[1] = x[0].y; ub[2] = x[1].x; ub[3] = x[1].y; ub[4] = x[2].x; ub[5] = x[2].y;
    w[0] = x[3].x; w[1] = x[3].y; w[2] = x[4].x;

    QA_SUBSTAMP(9);
    // ---- leg velocity, clamp, integrate
    float ul[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float g = w[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) g = fmaf(G[k * 6 + i], ub[i], g);
        float vl = tbl[T_VELLIM + k];
        ul[k] = clampf(g, -vl, vl);
    }
    V3 wb = v3(ub[0], ub[1], ub[2]);
    V3 wn = mul(R, wb), vn = mul(R, v3(ub[3], ub[4], ub[5]));
    st.pos = st.pos + dt * vn;
    {
        float wn2 = dot(wb, wb), wnorm = sqrtf(wn2), ang = wnorm * dt;
        float dx, dy, dz, dw;
        if (ang > 1e-12f) { float sh, ch; sincosf(0.5f * ang, &sh, &ch); float sc = sh / wnorm; dx = wb.x * sc; dy = wb.y * sc; dz = wb.z * sc; dw = ch; }
        else { dx = 0.5f * dt * wb.x; dy = 0.5f * dt * wb.y; dz = 0.5f * dt * wb.z; dw = 1.f; }
        float nx = st.qw * dx + st.qx * dw + st.qy * dz - st.qz * dy;
        float ny = st.qw * dy - st.qx * dz + st.qy * dw + st.qz * dx;
        float nz = st.qw * dz + st.qx * dy - st.qy * dx + st.qz * dw;
        float nw = st.qw * dw - st.qx * dx - st.qy * dy - st.qz * dz;
        float inv = rsqrtf(nx * nx + ny * ny + nz * nz + nw * nw);
        st.qx = nx * inv; st.qy = ny * inv; st.qz = nz * inv; st.qw = nw * inv;
    }
    st.vw = vn; st.ww = wn;
#pragma unroll
    for (int k = 0; k < 3; ++k) { st.q[k] = fmaf(dt, ul[k], st.q[k]); st.qd[k] = ul[k]; }

#pragma unroll
    for (int d = 0; d < 3; ++d) fimp[d] = foot_on ? rf[d].lam : 0.f;
    QA_SUBSTAMP(10);
    // ---- contact forces, world frame (plane: t1, t2, n are world x, y, z)
    float idt = 1.0f / dt;
    if (PLANE) co.foot_f = foot_on ? v3(rf[1].lam * idt, rf[2].lam * idt, rf[0].lam * idt) : v3(0, 0, 0);
    else if constexpr (SCH != 0) co.foot_f = foot_on ? sloped_contact_force(rf[0].lam, foot_n, rf[1].lam, ft1_w, rf[2].lam, ft2_w, idt) : v3(0, 0, 0);
    else co.foot_f = foot_on ? idt * ((rf[0].lam * foot_n) + (rf[1].lam * ft1_w) + (rf[2].lam * ft2_w)) : v3(0, 0, 0);    // lam_n n + lam_t1 t1 + lam_t2 t2, world frame
#pragma unroll
    for (int sl = 0; sl < QA_EXTRA_SLOTS; ++sl) {
        const bool on = any_extra[sl] && extra_on[sl];
        if (PLANE) co.extra_f[sl] = on ? v3(re_lam[sl][1] * idt, re_lam[sl][2] * idt, re_lam[sl][0] * idt) : v3(0, 0, 0);
        else if constexpr (SCH != 0) { V3 a, b; tangent_basis(ex_n[sl], a, b); co.extra_f[sl] = on ? sloped_contact_force(re_lam[sl][1], a, re_lam[sl][0], ex_n[sl], re_lam[sl][2], b, idt) : v3(0, 0, 0); }
        else { V3 a, b; tangent_basis(ex_n[sl], a, b); co.extra_f[sl] = on ? idt * ((re_lam[sl][0] * ex_n[sl]) + (re_lam[sl][1] * a) + (re_lam[sl][2] * b)) : v3(0, 0, 0); }
        co.extra_body[sl] = on ? ex_body[sl] : -1;
    }
    co.self_f = v3(0, 0, 0);
    if (P.self_collision) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) if (any_sc[pr] && sc_on[pr]) co.self_f = co.self_f + (sc_lam[pr] * idt) * mul(R, sc_nw[pr]);
    }
    if constexpr (SCH != 0) co.sh_lam = sh_lam;          // only ever changed under sh_on: 0 for a lane whose pair is apart
    if constexpr (SCH >= 2) { co.st_lam[0] = st_lam[0]; co.st_lam[1] = st_lam[1]; }
    // ---- what the contacts do to the articulated obstacles' joints: generalised force -f_n ca, summed over the quad, kept per env in LDS
    if (!PLANE && T.ob_acc) {
        float ga[QA_OBST_PER_ENV];
#pragma unroll
        for (int k = 0; k < QA_OBST_PER_ENV; ++k) {
            float g = (foot_on && foot_ob == k) ? -rf[0].lam * idt * foot_ca : 0.f;
#pragma unroll
            for (int sl = 0; sl < QA_EXTRA_SLOTS; ++sl) g += (any_extra[sl] && extra_on[sl] && ex_ob[sl] == k) ? -re_lam[sl][0] * idt * ex_ca[sl] : 0.f;
            ga[k] = quad_sum(g);
        }
        if (leg == 0) {
#pragma unroll
            for (int k = 0; k < QA_OBST_PER_ENV; ++k) T.ob_acc[k] += ga[k];
        }
    }
}

// joint dynamics of an articulated obstacle over one env step (h = decimation x dt) under the mean generalised contact force F of its
// substeps -- semi-implicit in the damper and the position drive, so the stiff bar / tyre drive (omega = 77 / 39 rad/s) is unconditionally
// stable at h = 20 ms.  See-saw: I q'' = F - c q', |q'| <= 8 rad/s, |q| <= asin(0.25 / 1.5) (inelastic stops).  Bar / tyre: m q'' = F - k q - c q'.
QA_DEV void obstacle_joint_step(float kind, float damping, float F, float h, float &q, float &qd) {
    if (kind == (float)QA_OBST_SEESAW) {
        qd = (qd + h * F / QA_SEESAW_INERTIA) / (1.0f + h * damping / QA_SEESAW_INERTIA);
        qd = clampf(qd, -QA_SEESAW_MAX_VEL, QA_SEESAW_MAX_VEL);
        q = fmaf(h, qd, q);
        if (q > QA_SEESAW_MAX_TILT) { q = QA_SEESAW_MAX_TILT; qd = 0.f; }
        if (q < -QA_SEESAW_MAX_TILT) { q = -QA_SEESAW_MAX_TILT; qd = 0.f; }
    } else if (kind != 0.f) {
        const float m = kind == (float)QA_OBST_BAR ? QA_BAR_MASS : QA_TYRE_MASS;
        qd = (qd + h * (F - QA_OBST_STIFFNESS * q) / m) / (1.0f + h * QA_OBST_DAMPING / m + h * h * QA_OBST_STIFFNESS / m);
        q = fmaf(h, qd, q);
    }
}

// joint origins + foot origin of a leg in the base frame (for RIGID_BODY_POS after the last substep)
QA_DEV void leg_origins(const float q[3], const float *tbl, V3 out[4]) {
    float s1, c1, s2, c2, s23, c23;
    __sincosf(q[0], &s1, &c1); __sincosf(q[1], &s2, &c2); __sincosf(q[1] + q[2], &s23, &c23);
    M3 R0, R1, R2;
    R0.m[0] = 1; R0.m[1] = 0; R0.m[2] = 0; R0.m[3] = 0; R0.m[4] = c1; R0.m[5] = -s1; R0.m[6] = 0; R0.m[7] = s1; R0.m[8] = c1;
    R1.m[0] = c2; R1.m[1] = 0; R1.m[2] = s2; R1.m[3] = s1 * s2; R1.m[4] = c1; R1.m[5] = -s1 * c2; R1.m[6] = -c1 * s2; R1.m[7] = s1; R1.m[8] = c1 * c2;
    R2.m[0] = c23; R2.m[1] = 0; R2.m[2] = s23; R2.m[3] = s1 * s23; R2.m[4] = c1; R2.m[5] = -s1 * c23; R2.m[6] = -c1 * s23; R2.m[7] = s1; R2.m[8] = c1 * c23;
    out[0] = v3(tbl[T_HIP_ORG], tbl[T_HIP_ORG + 1], tbl[T_HIP_ORG + 2]);
    out[1] = out[0] + mul(R0, v3(tbl[T_THIGH_ORG], tbl[T_THIGH_ORG + 1], tbl[T_THIGH_ORG + 2]));
    out[2] = out[1] + mul(R1, v3(tbl[T_CALF_ORG], tbl[T_CALF_ORG + 1], tbl[T_CALF_ORG + 2]));
    out[3] = out[2] + mul(R2, v3(tbl[T_FOOT_ORG], tbl[T_FOOT_ORG + 1], tbl[T_FOOT_ORG + 2]));
}
