// Frame renderer for play (contract: include/qa_render.h): a ray-cast of one env's robot -- the primitives of qa_render_shapes.h posed by
// QA_T_RIGID_BODY_STATE -- over the plane or the height field (+ ceiling map), K cameras in one launch, to shaded 8-bit RGB.
//
// One thread per pixel, 256-thread workgroups = a 16 x 16 pixel tile, grid (tiles, K).  The first 23 threads of a workgroup transform the
// env's primitives to the world frame into LDS once (20 floats each, 1,840 B); every ray tests a primitive's bounding sphere before the
// exact intersection.  Inside a wavefront the pixels that hit the robot finish early and the others walk the ground: at play sizes
// (one to sixteen 640 x 360 images) that divergence is not worth a compaction pass.
// The height field is NOT marched in fixed steps: the ray is cut at every line of the cell lattice it crosses (x lines, y lines and the
// cells' diagonals), between two cuts the two-triangle surface is one plane, and the crossing inside that piece is closed form.  The cell
// lookup is the depth camera's (cell_of / tri_height of qa_depth.hip, restated here: that file's images are pinned bit for bit and it
// shares no source with this one).
// The helpers live in qa_render_walk.h, shared with the course mode (qa_render_course.hip), to which qa_render_frames hands a call with
// QA_RENDER_COURSE set once the common arguments are checked.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/qa_render_course.h"
#include "qa_render_walk.h"

extern thread_local char qa_err_buf[512];

// qa_render_course.hip: checks the course members of an otherwise checked call, then launches qa_render_course_kernel; `light` is the unit light_dir
__attribute__((visibility("hidden"))) int qa_render_course_launch(const qa_render_cfg *cfg, const qa_render_course *course, const float *light, void *stream);

namespace {

__global__ void __launch_bounds__(256) qa_render_kernel(RenderArgs a) {
    const qa_render_cfg &c = a.c;
    __shared__ float s_prim[QA_RS_NUM_PRIMS * PRIM_FLOATS];
    const int k = blockIdx.y;
    const int e = min(max(a.io.env_ids[k], 0), c.num_envs - 1);
    if (threadIdx.x < QA_RS_NUM_PRIMS) stage_prim(QA_RS_TABLE_DEV, a.io.body_state + (int64_t)e * (QA_RS_NUM_BODIES * 13), threadIdx.x, s_prim + threadIdx.x * PRIM_FLOATS);
    __syncthreads();
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int i = tile_y * 16 + (threadIdx.x >> 4), j = tile_x * 16 + (threadIdx.x & 15);
    if (i >= c.height || j >= c.width) return;                               // (after the barrier: the lanes of a partial tile took part in it)

    const float *cam = a.io.cameras + k * 7;
    const float o[3] = {cam[0], cam[1], cam[2]};
    float f[3] = {cam[3] - o[0], cam[4] - o[1], cam[5] - o[2]};
    const float ifl = 1.0f / sqrtf(qa_rs_dot(f, f));
    f[0] *= ifl; f[1] *= ifl; f[2] *= ifl;
    float r[3] = {f[1], -f[0], 0.f};                                          // f x (0, 0, 1)
    float rl = r[0] * r[0] + r[1] * r[1];
    if (rl < 1e-12f) { r[0] = 0.f; r[1] = f[2]; r[2] = -f[1]; rl = r[1] * r[1] + r[2] * r[2]; }   // straight up / down: f x (1, 0, 0)
    const float irl = 1.0f / sqrtf(rl);
    r[0] *= irl; r[1] *= irl; r[2] *= irl;
    const float u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};   // r x f
    const float tv = tanf(0.5f * cam[6]), th = tv * (float)c.width / (float)c.height;
    const float sx = (((float)j + 0.5f) / (float)c.width * 2.0f - 1.0f) * th;
    const float sy = (1.0f - ((float)i + 0.5f) / (float)c.height * 2.0f) * tv;
    float d[3] = {f[0] + sx * r[0] + sy * u[0], f[1] + sx * r[1] + sy * u[1], f[2] + sx * r[2] + sy * u[2]};
    const float idl = 1.0f / sqrtf(qa_rs_dot(d, d));
    d[0] *= idl; d[1] *= idl; d[2] *= idl;

    float t = c.far, n[3] = {0.f, 0.f, 1.f};
    int id = QA_RENDER_ID_SKY, cls = QA_RS_CLS_SKY;
    const int pi = robot_hit(QA_RS_TABLE_DEV, s_prim, o, d, c.far, &t, n);
    if (pi >= 0) { id = QA_RS_TABLE_DEV[pi].body; cls = QA_RS_TABLE_DEV[pi].cls; }

    if (c.terrain_type == 0) {
        if (d[2] < 0.f && o[2] > 0.f) {
            const float tg = -o[2] / d[2];
            if (tg < t) { t = tg; id = QA_RENDER_ID_GROUND; cls = QA_RS_CLS_GROUND; n[0] = 0.f; n[1] = 0.f; n[2] = 1.f; }
        }
    } else {
        const int rows = c.map_rows, cols = c.map_cols;
        const int16_t *hm = a.io.height_samples, *cm = a.io.ceiling_samples;
        const float fx0 = (o[0] + c.border_size) * a.inv_hs, fy0 = (o[1] + c.border_size) * a.inv_hs;
        const float dfx = d[0] * a.inv_hs, dfy = d[1] * a.inv_hs;
        Line lx = line_init(fx0, dfx), ly = line_init(fy0, dfy), ld = line_init(fx0 - fy0, dfx - dfy);
        float tx = line_t(lx), ty = line_t(ly), td = line_t(ld);
        const float tend = t;                                               // nothing behind the robot's hit (or `far`) is looked at
        float ta = 0.f;
        while (ta < tend) {
            const float tb = fminf(fminf(tx, ty), fminf(td, tend));
            const float tm = 0.5f * (ta + tb);
            const float fxm = fx0 + tm * dfx, fym = fy0 + tm * dfy;
            const float fxa = fx0 + ta * dfx, fya = fy0 + ta * dfy, fxb = fx0 + tb * dfx, fyb = fy0 + tb * dfy;
            const float za = o[2] + ta * d[2], zb = o[2] + tb * d[2];
            float th_ = 3.0e38f;
            const Piece pf = piece_at(hm, rows, cols, c.vertical_scale, fxm, fym);
            const float ga = za - piece_height(pf, fxa, fya), gb = zb - piece_height(pf, fxb, fyb);
            if (ga >= 0.f && gb < 0.f) {                                     // from above, inside this piece: the plane's crossing
                th_ = ta + (tb - ta) * (ga / (ga - gb));
                id = QA_RENDER_ID_GROUND; cls = QA_RS_CLS_GROUND;
                piece_normal(pf, fxm, fym, rows, cols, a.inv_hs, n);
            }
            if (cm) {
                const Piece pc = piece_at(cm, rows, cols, c.vertical_scale, fxm, fym);
                if (pc.exists) {
                    const float ha = za - piece_height(pc, fxa, fya), hb = zb - piece_height(pc, fxb, fyb);
                    if ((ha < 0.f) != (hb < 0.f)) {                          // a thin shell: from below or from above
                        const float tc = ta + (tb - ta) * (ha / (ha - hb));
                        if (tc < th_) {
                            th_ = tc; id = QA_RENDER_ID_CEILING; cls = QA_RS_CLS_CEILING;
                            piece_normal(pc, fxm, fym, rows, cols, a.inv_hs, n);
                            if (ha < 0.f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }     // seen from below: the underside
                        }
                    }
                }
            }
            if (th_ < 1.0e38f) { t = fminf(th_, tend); break; }
            if (tx <= tb) { lx.m += lx.step; tx = line_t(lx); }
            if (ty <= tb) { ly.m += ly.step; ty = line_t(ly); }
            if (td <= tb) { ld.m += ld.step; td = line_t(ld); }
            ta = tb;
        }
    }

    float col[3] = {PALETTE_DEV[cls][0], PALETTE_DEV[cls][1], PALETTE_DEV[cls][2]};
    if (id != QA_RENDER_ID_SKY) {
        const float hp[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        float lam = fmaxf(qa_rs_dot(n, a.light), 0.f);
        if (id == QA_RENDER_ID_GROUND) {
            if ((c.flags & QA_RENDER_CHECKER) && (((int)floorf(hp[0] * (1.0f / QA_RENDER_CHECKER_SIZE)) + (int)floorf(hp[1] * (1.0f / QA_RENDER_CHECKER_SIZE))) & 1)) {
                col[0] *= QA_RENDER_CHECKER_DARK; col[1] *= QA_RENDER_CHECKER_DARK; col[2] *= QA_RENDER_CHECKER_DARK;
            }
            if ((c.flags & QA_RENDER_SHADOWS) && lam > 0.f) {
                float ts, ns[3];
                if (robot_hit(QA_RS_TABLE_DEV, s_prim, hp, a.light, 3.0e38f, &ts, ns) >= 0) lam = 0.f;
            }
        }
        const float shade = QA_RENDER_AMBIENT + (1.0f - QA_RENDER_AMBIENT) * lam;
        col[0] *= shade; col[1] *= shade; col[2] *= shade;
    }
    const int64_t px = ((int64_t)k * c.height + i) * c.width + j;
    uint8_t *out = a.io.rgb + px * 3;
    for (int q = 0; q < 3; ++q) out[q] = (uint8_t)fminf(fmaxf(col[q] * 255.0f + 0.5f, 0.f), 255.f);
    if (a.io.depth) a.io.depth[px] = t;
    if (a.io.ids) a.io.ids[px] = (int8_t)id;
}

}  // namespace

#define RENDER_FAIL(...) do { snprintf(qa_err_buf, sizeof(qa_err_buf), __VA_ARGS__); return QA_E_ARG; } while (0)

extern "C" int qa_render_frames(const qa_render_cfg *cfg, const qa_render_io *io, void *stream) {
    if (!cfg || !io) RENDER_FAIL("qa_render_frames: null argument");
    if (cfg->num_cameras < 1) RENDER_FAIL("qa_render_frames: num_cameras = %d, nothing to render", cfg->num_cameras);
    if (cfg->num_envs < 1) RENDER_FAIL("qa_render_frames: num_envs = %d", cfg->num_envs);
    if (cfg->width < 1 || cfg->height < 1) RENDER_FAIL("qa_render_frames: image size %d x %d", cfg->width, cfg->height);
    if ((int64_t)cfg->num_cameras * cfg->width * cfg->height * 3 > (int64_t)INT32_MAX) RENDER_FAIL("qa_render_frames: %d images of %d x %d overflow a 32-bit pixel count", cfg->num_cameras, cfg->width, cfg->height);
    if (!io->rgb || !io->body_state || !io->env_ids || !io->cameras) RENDER_FAIL("qa_render_frames: rgb, body_state, env_ids and cameras are required");
    if (cfg->terrain_type != 0 && cfg->terrain_type != 1) RENDER_FAIL("qa_render_frames: terrain_type %d (0 = plane, 1 = height field)", cfg->terrain_type);
    if (cfg->terrain_type == 1 && (!io->height_samples || cfg->map_rows < 2 || cfg->map_cols < 2 || !(cfg->horizontal_scale > 0.f)))
        RENDER_FAIL("qa_render_frames: terrain_type 1 needs height_samples, map_rows / map_cols >= 2 and horizontal_scale > 0");
    if (!(cfg->far > 0.f)) RENDER_FAIL("qa_render_frames: far = %g", (double)cfg->far);
    // a ray crosses at most ~2.4 lattice lines per cell of its length: the cap keeps every argument's walk finite (and its line indices in int32)
    if (cfg->terrain_type == 1 && !(cfg->far / cfg->horizontal_scale <= 1.0e6f)) RENDER_FAIL("qa_render_frames: far = %g is more than 1e6 cells of %g m", (double)cfg->far, (double)cfg->horizontal_scale);
    const double ll = sqrt((double)cfg->light_dir[0] * cfg->light_dir[0] + (double)cfg->light_dir[1] * cfg->light_dir[1] + (double)cfg->light_dir[2] * cfg->light_dir[2]);
    if (!(ll > 0.0)) RENDER_FAIL("qa_render_frames: light_dir is zero");
    if (io->env_ids_host)
        for (int k = 0; k < cfg->num_cameras; ++k)
            if (io->env_ids_host[k] < 0 || io->env_ids_host[k] >= cfg->num_envs) RENDER_FAIL("qa_render_frames: env_ids[%d] = %d is outside [0, %d)", k, io->env_ids_host[k], cfg->num_envs);
    RenderArgs a; a.c = *cfg; a.io = *io;
    for (int q = 0; q < 3; ++q) a.light[q] = (float)(cfg->light_dir[q] / ll);
    a.inv_hs = cfg->terrain_type == 1 ? 1.0f / cfg->horizontal_scale : 0.f;
    a.tiles_x = (cfg->width + 15) / 16;
    const int tiles_y = (cfg->height + 15) / 16;
    if (cfg->num_cameras > 65535) RENDER_FAIL("qa_render_frames: num_cameras = %d (at most 65535 per launch)", cfg->num_cameras);
    if (cfg->flags & QA_RENDER_COURSE) return qa_render_course_launch(cfg, (const qa_render_course *)io, a.light, stream);
    hipLaunchKernelGGL(qa_render_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)cfg->num_cameras), dim3(256), 0, (hipStream_t)stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) { snprintf(qa_err_buf, sizeof(qa_err_buf), "qa_render_frames: %s", hipGetErrorString(err)); return QA_E_DEVICE; }
    return QA_OK;
}

extern "C" int qa_render_shape_table(float *out, int cap) {
    for (int i = 0; i < QA_RS_NUM_PRIMS && i < cap && out; ++i) {
        const qa_rs_prim &p = QA_RS_TABLE[i];
        float *w = out + 10 * i;
        w[0] = (float)p.kind; w[1] = (float)p.body; w[2] = (float)p.cls;
        for (int q = 0; q < 3; ++q) { w[3 + q] = p.a[q]; w[6 + q] = p.b[q]; }
        w[9] = p.r;
    }
    return QA_RS_NUM_PRIMS;
}

extern "C" int qa_render_palette(float *out) {
    for (int i = 0; i < QA_RS_NUM_CLASSES; ++i)
        for (int q = 0; q < 3; ++q) out[3 * i + q] = PALETTE[i][q];
    return QA_RS_NUM_CLASSES;
}

extern "C" int qa_render_sizeof(int which) { return which == 0 ? (int)sizeof(qa_render_cfg) : (int)sizeof(qa_render_io); }
