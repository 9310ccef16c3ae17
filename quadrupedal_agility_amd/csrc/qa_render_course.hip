// The course mode of the frame renderer (contract: include/qa_render_course.h): qa_render_frames with QA_RENDER_COURSE ends here.  The
// see-saw, bar and tyre are drawn in their joint state -- the surface of qa_obst_surface.h, which the physics and the depth camera share --
// and the env's goals as spheres.  A unit of its own: qa_render_kernel (qa_render.hip) keeps its device code, instruction for instruction.
//
// The launch has qa_render_kernel's shape: one thread per pixel, 256-thread workgroups = a 16 x 16 pixel tile, grid (tiles, K).  Threads
// 0..22 stage the robot's primitives as there; threads 64..99 stage the env's 3 x 12 record floats (tan q in float 10, qa_os_record_float)
// and threads 128..223 the goal centres, so that the three run side by side in different wavefronts; one barrier, before the lanes of a
// partial tile leave.  The pixel itself is qa_rc_pixel of qa_render_course_walk.h, which the host twin compiles too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "qa_render_course_walk.h"

extern thread_local char qa_err_buf[512];

namespace {

struct CourseArgs {
    qa_render_cfg c;
    qa_render_course io;
    float light[3];         // unit
    float inv_hs;
    int tiles_x;
};

constexpr int REC_FLOATS = QA_OS_SLOTS * QA_OS_RECORD, REC_THREAD0 = 64, GOAL_THREAD0 = 128;
static_assert(QA_RS_NUM_PRIMS <= REC_THREAD0 && REC_THREAD0 + REC_FLOATS <= GOAL_THREAD0 && GOAL_THREAD0 + 3 * QA_RENDER_MAX_GOALS <= 256, "staging threads overlap");

__global__ void __launch_bounds__(256) qa_render_course_kernel(CourseArgs a) {
    const qa_render_cfg &c = a.c;
    __shared__ float s_prim[QA_RS_NUM_PRIMS * PRIM_FLOATS];
    __shared__ float s_rec[REC_FLOATS];
    __shared__ float s_goal[3 * QA_RENDER_MAX_GOALS];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int e = min(max(a.io.io.env_ids[k], 0), c.num_envs - 1);
    const int num_goals = a.io.goals ? a.io.num_goals : 0;
    if (tid < QA_RS_NUM_PRIMS) stage_prim(QA_RS_TABLE_DEV, a.io.io.body_state + (int64_t)e * (QA_RS_NUM_BODIES * 13), tid, s_prim + tid * PRIM_FLOATS);
    else if (tid >= REC_THREAD0 && tid < REC_THREAD0 + REC_FLOATS) {
        const int q = tid - REC_THREAD0;                                    // without obstacles: three empty slots (kind 0)
        s_rec[q] = a.io.obst_desc ? qa_os_record_float(a.io.obst_desc + (int64_t)e * (QA_OS_SLOTS * 8), a.io.obst_state + (int64_t)e * (QA_OS_SLOTS * 4), q / QA_OS_RECORD, q % QA_OS_RECORD) : 0.f;
    } else if (tid >= GOAL_THREAD0 && tid < GOAL_THREAD0 + 3 * num_goals)
        s_goal[tid - GOAL_THREAD0] = a.io.goals[(int64_t)e * (3 * num_goals) + (tid - GOAL_THREAD0)];
    __syncthreads();
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int i = tile_y * 16 + (tid >> 4), j = tile_x * 16 + (tid & 15);
    if (i >= c.height || j >= c.width) return;                               // (after the barrier: the lanes of a partial tile took part in it)

    const int cur_goal = a.io.cur_goal_idx ? (int)a.io.cur_goal_idx[e] : -1;
    const int reached = a.io.reached ? (int)a.io.reached[e] : 0;
    float o[3], d[3], t, col[3];
    qa_rc_pixel_ray(a.io.io.cameras + k * 7, c.width, c.height, i, j, o, d);
    const int id = qa_rc_pixel(QA_RS_TABLE_DEV, &PALETTE_DEV[0][0], s_prim, s_rec, s_goal, num_goals, a.io.goal_radius, cur_goal, reached, a.io.io.height_samples, a.io.io.ceiling_samples,
                               c.map_rows, c.map_cols, c.border_size, a.inv_hs, c.vertical_scale, c.far, a.light, c.flags, o, d, &t, col);
    const int64_t px = ((int64_t)k * c.height + i) * c.width + j;
    uint8_t *out = a.io.io.rgb + px * 3;
    for (int q = 0; q < 3; ++q) out[q] = (uint8_t)fminf(fmaxf(col[q] * 255.0f + 0.5f, 0.f), 255.f);
    if (a.io.io.depth) a.io.io.depth[px] = t;
    if (a.io.io.ids) a.io.io.ids[px] = (int8_t)id;
}

}  // namespace

#define COURSE_FAIL(...) do { snprintf(qa_err_buf, sizeof(qa_err_buf), __VA_ARGS__); return QA_E_ARG; } while (0)

__attribute__((visibility("hidden"))) int qa_render_course_launch(const qa_render_cfg *cfg, const qa_render_course *course, const float *light, void *stream) {
    if (cfg->terrain_type != 1)
        COURSE_FAIL("qa_render_frames: QA_RENDER_COURSE draws the height field's obstacles and goals: terrain_type %d is not 1", cfg->terrain_type);
    if (!course->obst_desc != !course->obst_state) COURSE_FAIL("qa_render_frames: QA_RENDER_COURSE takes obst_desc and obst_state together");
    if (!course->obst_desc && !course->goals) COURSE_FAIL("qa_render_frames: QA_RENDER_COURSE with neither obstacles nor goals: clear the flag");
    if (course->goals && (course->num_goals < 1 || course->num_goals > QA_RENDER_MAX_GOALS))
        COURSE_FAIL("qa_render_frames: num_goals = %d is outside [1, %d]", course->num_goals, QA_RENDER_MAX_GOALS);
    if (course->goals && !(course->goal_radius > 0.f)) COURSE_FAIL("qa_render_frames: goal_radius = %g", (double)course->goal_radius);
    CourseArgs a; a.c = *cfg; a.io = *course;
    for (int q = 0; q < 3; ++q) a.light[q] = light[q];
    a.inv_hs = 1.0f / cfg->horizontal_scale;
    a.tiles_x = (cfg->width + 15) / 16;
    const int tiles_y = (cfg->height + 15) / 16;
    hipLaunchKernelGGL(qa_render_course_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)cfg->num_cameras), dim3(256), 0, (hipStream_t)stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) { snprintf(qa_err_buf, sizeof(qa_err_buf), "qa_render_frames: %s", hipGetErrorString(err)); return QA_E_DEVICE; }
    return QA_OK;
}
