// Host twin of the calf-against-neighbouring-hip geometry (include/qa_sim_selfcol.h): the SAME inline functions phys_substep (qa_physics.h)
// calls -- quadrupedal_agility_amd/csrc/qa_selfcol.h -- driven from plain C++ on arrays, so that tests/test_selfcol_hips_cpu.py checks gap,
// normal and closest-point parameters against a float64 closed form without a GPU.
// Built by that test as a shared library: c++ -O2 -std=c++17 -shared -fPIC.  Row-major arrays.
#include <stdint.h>

#include "../../quadrupedal_agility_amd/csrc/qa_selfcol.h"

// hip capsule segments of n legs: org (n,3) hip joint origins, q0 (n) joint-0 angles, side (n) +1 left / -1 right -> h0, h1 (n,3)
extern "C" int qa_selfcol_hip_segment_host(int n, const float *org, const float *q0, const float *side, float *h0, float *h1) {
    if (n <= 0) return -1;
    for (int i = 0; i < n; ++i) qa_sc_hip_segment(org + 3 * i, cosf(q0[i]), sinf(q0[i]), side[i], h0 + 3 * i, h1 + 3 * i);
    return 0;
}

// What one LANE of a pair computes.  A lane owns one side of the relation (own_is_calf: its calf capsule own0 = knee, own1 = foot; else its hip
// capsule own0, own1) and has fetched the other side's two points (other0, other1).  It orders the operands by role (calf first), as the kernel
// does, and reports the normal as the direction of the force on ITS body.  Calling it for the two lanes of a pair -- (own, other, 1) and
// (other, own, 0) -- must give bit-identical gap, s and t and negated normals.
extern "C" int qa_selfcol_lane_host(int n, const float *own0, const float *own1, const float *other0, const float *other1, const int32_t *own_is_calf,
                                    float *gap /* (n) */, float *normal /* (n,3) */, float *s /* (n) */, float *t /* (n) */, float *own_point /* (n,3) */) {
    if (n <= 0) return -1;
    for (int i = 0; i < n; ++i) {
        const bool calf = own_is_calf[i] != 0;
        const float *c0 = (calf ? own0 : other0) + 3 * i, *c1 = (calf ? own1 : other1) + 3 * i;
        const float *h0 = (calf ? other0 : own0) + 3 * i, *h1 = (calf ? other1 : own1) + 3 * i;
        qa_sc_contact ct;
        qa_sc_calf_hip(c0, c1, h0, h1, &ct);
        const float sg = calf ? 1.f : -1.f;
        gap[i] = ct.gap; s[i] = ct.s; t[i] = ct.t;
        for (int k = 0; k < 3; ++k) { normal[3 * i + k] = sg * ct.n[k]; own_point[3 * i + k] = calf ? ct.pc[k] : ct.ph[k]; }
    }
    return 0;
}
