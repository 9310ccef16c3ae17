// Host twin of quadrupedal_agility_amd/csrc/qa_render_shapes.h: the header's three ray-primitive functions and its table, compiled with the
// host compiler and called through ctypes by tests/test_render_cpu.py (which compares them with the float64 reference tests/render_ref.py).
#include <stdint.h>

#include "../../quadrupedal_agility_amd/csrc/qa_render_shapes.h"

extern "C" {

// kind = QA_RS_*; rays (n,6): origin, unit direction; prim (n,16): a[3], b[3], r, R[9] (row-major, boxes); out (n,5): hit, t, normal
int qa_render_shapes_host(int kind, int n, const float *rays, const float *prim, float *out) {
    for (int i = 0; i < n; ++i) {
        const float *ry = rays + 6 * i, *p = prim + 16 * i;
        float t = 0.f, nn[3] = {0.f, 0.f, 0.f};
        int hit;
        if (kind == QA_RS_SPHERE) hit = qa_rs_ray_sphere(ry, ry + 3, p, p[6], &t, nn);
        else if (kind == QA_RS_CAPSULE) hit = qa_rs_ray_capsule(ry, ry + 3, p, p + 3, p[6], &t, nn);
        else if (kind == QA_RS_BOX) hit = qa_rs_ray_box(ry, ry + 3, p, p + 7, p + 3, &t, nn);
        else return -1;
        float *o = out + 5 * i;
        o[0] = (float)hit; o[1] = hit ? t : 0.f; o[2] = nn[0]; o[3] = nn[1]; o[4] = nn[2];
    }
    return 0;
}

// the header's table as 10 floats per primitive (kind, body, class, a, b, r); returns the count
int qa_render_shapes_table_host(float *out, int cap) {
    for (int i = 0; i < QA_RS_NUM_PRIMS && i < cap; ++i) {
        const qa_rs_prim &p = QA_RS_TABLE[i];
        float *w = out + 10 * i;
        w[0] = (float)p.kind; w[1] = (float)p.body; w[2] = (float)p.cls;
        for (int q = 0; q < 3; ++q) { w[3 + q] = p.a[q]; w[6 + q] = p.b[q]; }
        w[9] = p.r;
    }
    return QA_RS_NUM_PRIMS;
}

void qa_render_quat_matrix_host(const float *q, float *R) { qa_rs_quat_matrix(q, R); }
}
