// Host twin of the articulated obstacles' rendered surface (qa_tsc_depth_update_obstacles, include/qa_tsc_depth_obstacles.h): the SAME inline
// functions the depth ray-cast (qa_depth.hip) calls -- quadrupedal_agility_amd/csrc/qa_obst_surface.h -- driven from plain C++ on arrays, so
// that tests/test_depth_obstacles_cpu.py checks footprint, floor, ceiling and the skip boxes against float64 (tests/depth_obstacles_ref.py)
// without a GPU.  Built by that test as a shared library: c++ -O2 -std=c++17 -shared -fPIC.  Row-major arrays.
//
// With -DQA_OBST_SURFACE_HOST_MAIN it is a program: it reads, from the file named by its argument or from stdin, 24 floats of one env's
// QA_T_OBST_DESC rows, 12 floats of its QA_T_OBST_STATE rows, then any number of points "x y map_floor map_ceiling", and prints
// "mode floor ceiling" per point.
#include <stdint.h>
#include <stdio.h>

#include "../../quadrupedal_agility_amd/csrc/qa_obst_surface.h"

// the record as the kernel stages it: float j of slot k, for all 36
extern "C" int qa_obst_surface_record_host(const float *desc /* (3,8) */, const float *state /* (3,4) */, float *rec /* (3,12) */) {
    for (int i = 0; i < QA_OS_SLOTS * QA_OS_RECORD; ++i) rec[i] = qa_os_record_float(desc, state, i / QA_OS_RECORD, i % QA_OS_RECORD);
    return 0;
}

// n points against one env's records
extern "C" int qa_obst_surface_host(int n, const float *desc, const float *state, const float *x, const float *y, const float *map_floor,
                                    const float *map_ceiling, int32_t *mode /* (n) */, float *floor_out /* (n) */, float *ceiling_out /* (n) */) {
    if (n <= 0) return -1;
    float rec[QA_OS_SLOTS * QA_OS_RECORD];
    qa_obst_surface_record_host(desc, state, rec);
    for (int i = 0; i < n; ++i) {
        const qa_os_cover c = qa_os_classify(rec, x[i], y[i]);
        mode[i] = c.mode; floor_out[i] = qa_os_floor(&c, map_floor[i]); ceiling_out[i] = qa_os_ceiling(&c, map_ceiling[i]);
    }
    return 0;
}

// the three skip boxes (3,4) of one env, and whether the rectangle [x_lo, x_hi] x [y_lo, y_hi] overlaps one of them
extern "C" int qa_obst_surface_boxes_host(const float *desc, float *boxes, float x_lo, float x_hi, float y_lo, float y_hi) {
    for (int k = 0; k < QA_OS_SLOTS; ++k) qa_os_box(desc, k, boxes + 4 * k);
    return qa_os_boxes_overlap(boxes, x_lo, x_hi, y_lo, y_hi) ? 1 : 0;
}

// does the ray (ox, oy) + t (dx, dy), 0 <= t <= t_max, pass over one of the env's three boxes (the kernel's test for "render this pixel again")
extern "C" int qa_obst_surface_ray_host(const float *desc, float ox, float oy, float dx, float dy, float t_max) {
    float boxes[QA_OS_SLOTS * 4];
    for (int k = 0; k < QA_OS_SLOTS; ++k) qa_os_box(desc, k, boxes + 4 * k);
    return qa_os_ray_meets_boxes(boxes, ox, oy, dx, dy, dx != 0.f ? 1.0f / dx : 0.f, dy != 0.f ? 1.0f / dy : 0.f, t_max) ? 1 : 0;
}

#ifdef QA_OBST_SURFACE_HOST_MAIN
int main(int argc, char **argv) {
    FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) { fprintf(stderr, "qa_obst_surface_host: cannot open %s\n", argv[1]); return 2; }
    float desc[QA_OS_SLOTS * 8], state[QA_OS_SLOTS * 4];
    for (float &v : desc) if (fscanf(in, "%f", &v) != 1) { fprintf(stderr, "qa_obst_surface_host: 24 descriptor floats expected\n"); return 2; }
    for (float &v : state) if (fscanf(in, "%f", &v) != 1) { fprintf(stderr, "qa_obst_surface_host: 12 state floats expected\n"); return 2; }
    float x, y, mf, mc;
    while (fscanf(in, "%f %f %f %f", &x, &y, &mf, &mc) == 4) {
        int32_t mode; float fl, ce;
        qa_obst_surface_host(1, desc, state, &x, &y, &mf, &mc, &mode, &fl, &ce);
        printf("%d %.9g %.9g\n", (int)mode, fl, ce);
    }
    if (in != stdin) fclose(in);
    return 0;
}
#endif
