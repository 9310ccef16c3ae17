// Host twin of quadrupedal_agility_amd/csrc/qa_render_course_walk.h: the course renderer's pixel function -- cuts, pieces, the face rule,
// goals and shading -- compiled with the host compiler and run over whole images on plain arrays, as qa_render_course_kernel runs it on the
// staged arrays in LDS.  tests/test_render_course_cpu.py calls it through ctypes and holds it to the float64 reference
// tests/render_course_ref.py.  With QA_RENDER_COURSE_HOST_MAIN it is a stand-alone program (one small scene, a checksum), for a sanitizer build.
#include <stdint.h>
#include <stdio.h>

#include "../../quadrupedal_agility_amd/csrc/qa_render_course_walk.h"

extern "C" {

// One camera.  body (19,13) rows of the env; desc (3,8) / state (3,4) of the env or NULL; goals (num_goals,3) of the env (num_goals 0: none);
// cam[7]; maps (rows, cols), cm may be NULL; geo = border, horizontal_scale, vertical_scale, far; light: unit.
// Writes rgb (H,W,3) uint8, depth (H,W), ids (H,W) int8.
int qa_render_course_host(const float *body, const float *desc, const float *state, const float *goals, int num_goals, float goal_radius, int cur_goal,
                          int reached, const float *cam, const int16_t *hm, const int16_t *cm, int rows, int cols, const float *geo, const float *light,
                          int flags, int width, int height, uint8_t *rgb, float *depth, int8_t *ids) {
    if (num_goals < 0 || num_goals > QA_RENDER_MAX_GOALS) return -1;
    float prims[QA_RS_NUM_PRIMS * PRIM_FLOATS], rec[QA_OS_SLOTS * QA_OS_RECORD];
    for (int i = 0; i < QA_RS_NUM_PRIMS; ++i) stage_prim(QA_RS_TABLE, body, i, prims + i * PRIM_FLOATS);
    for (int q = 0; q < QA_OS_SLOTS * QA_OS_RECORD; ++q) rec[q] = desc ? qa_os_record_float(desc, state, q / QA_OS_RECORD, q % QA_OS_RECORD) : 0.f;
    const float inv_hs = 1.0f / geo[1];
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j) {
            float o[3], d[3], t, col[3];
            qa_rc_pixel_ray(cam, width, height, i, j, o, d);
            const int id = qa_rc_pixel(QA_RS_TABLE, &PALETTE[0][0], prims, rec, goals, num_goals, goal_radius, cur_goal, reached, hm, cm, rows, cols, geo[0], inv_hs, geo[2], geo[3], light,
                                       flags, o, d, &t, col);
            const int px = i * width + j;
            for (int q = 0; q < 3; ++q) rgb[3 * px + q] = (uint8_t)fminf(fmaxf(col[q] * 255.0f + 0.5f, 0.f), 255.f);
            depth[px] = t; ids[px] = (int8_t)id;
        }
    return 0;
}

}

#ifdef QA_RENDER_COURSE_HOST_MAIN
// a see-saw at its stop, a raised bar and a lowered tyre on a flat 24 x 24 map with a ceiling strip, three goals, a robot parked in view
int main() {
    enum { ROWS = 24, COLS = 24, W = 61, H = 35 };
    static int16_t hm[ROWS * COLS], cm[ROWS * COLS];
    for (int i = 0; i < ROWS * COLS; ++i) { hm[i] = 0; cm[i] = QA_NO_CEILING; }
    for (int i = 10; i < 14; ++i) for (int j = 4; j < 20; ++j) { hm[i * COLS + j] = 60; cm[i * COLS + j] = 200; }
    float body[19 * 13] = {0};
    for (int b = 0; b < 19; ++b) { body[13 * b] = 1.0f + 0.05f * b; body[13 * b + 1] = 1.5f; body[13 * b + 2] = 0.4f; body[13 * b + 6] = 1.f; }
    const float desc[24] = {2.f, 2.f, 0.8253356f, 0.5646425f, 1.2f, 0.3f, 0.26f, 1.f,  1.f, 3.f, 1.f, 0.f, 0.3f, 1.5f, 0.f, 2.f,  4.f, 3.f, 1.f, 0.f, 0.5f, 0.5f, 0.f, 3.f};
    const float state[12] = {0.21f, 0.f, 0.f, 0.f,  0.05f, 0.f, 0.f, 0.f,  -0.05f, 0.f, 0.f, 0.f};
    const float goals[9] = {2.f, 2.f, 0.6f, 3.f, 1.f, 0.f, -4.f, -4.f, 0.f};
    const float cam[7] = {-0.6f, 0.3f, 1.4f, 2.2f, 2.3f, 0.2f, 1.0f}, geo[4] = {1.0f, 0.25f, 0.005f, 20.f}, light[3] = {0.30929f, 0.22092f, 0.92493f};
    static uint8_t rgb[W * H * 3]; static float depth[W * H]; static int8_t ids[W * H];
    if (qa_render_course_host(body, desc, state, goals, 3, 0.1f, 0, 1, cam, hm, cm, ROWS, COLS, geo, light, 3, W, H, rgb, depth, ids)) return 1;
    long sum = 0; int seen[32] = {0};
    for (int i = 0; i < W * H; ++i) { sum += rgb[3 * i] + rgb[3 * i + 1] + rgb[3 * i + 2]; seen[ids[i] + 1] = 1; }
    printf("checksum %ld, ids:", sum);
    for (int i = 0; i < 32; ++i) if (seen[i]) printf(" %d", i - 1);
    printf("\n");
    return 0;
}
#endif
