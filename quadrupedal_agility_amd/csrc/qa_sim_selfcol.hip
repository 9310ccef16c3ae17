// qa_sim_selfcol.hip -- the SCH = 1 instantiations of the kernels that run physics (qa_set_self_collision_hips, include/qa_sim_selfcol.h): the env
// step of every export mode on the plane (with and without helper wavefronts) and on the height field, the physics-only step of the task-level
// tree, and qa_simulate / qa_simulate_if.  They are the templates of qa_sim.hip, compiled in a translation unit of their own so that the kernels
// without the calf-hip rows keep the code they had (see the note at the top of qa_sim.hip); qa_sim.hip's host side reaches them through the
// four functions below.  qa_sim_selfcol_thighs.hip includes THIS file with QA_SCH_LEVEL 2: the same launchers over the SCH = 2 instantiations
// (qa_set_self_collision_thighs), as qa_sct_*, in a third translation unit.
#define QA_SIM_SCH_TU
#ifndef QA_SCH_LEVEL
#define QA_SCH_LEVEL 1
#define QA_SCH_FN(name) qa_sch_##name
#endif
#include "qa_sim.hip"

int QA_SCH_FN(upload_table)(const float *tbl, size_t bytes) {
    if (bytes != sizeof(float) * QA_TBL_FLOATS) return QA_E_ARG;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_tbl), tbl, bytes);
    return e == hipSuccess ? QA_OK : fail_hip(e, "hipMemcpyToSymbol(c_tbl, self-collision kernels)");
}

void QA_SCH_FN(launch_env_step)(bool hf, int lean, bool helpers, bool xr, int blocks, hipStream_t st, const StepArgs &a) {
#define QA_LAUNCH_STEP(PLANE_, LEAN_, HELP_) do { \
        if (xr) hipLaunchKernelGGL((qa_env_step_kernel<PLANE_, 4, 0, LEAN_, HELP_, 1, QA_SCH_LEVEL>), dim3(blocks), dim3((HELP_ ? 3 : 1) * QA_BLOCK), 0, st, a); \
        else hipLaunchKernelGGL((qa_env_step_kernel<PLANE_, 4, 0, LEAN_, HELP_, 0, QA_SCH_LEVEL>), dim3(blocks), dim3((HELP_ ? 3 : 1) * QA_BLOCK), 0, st, a); } while (0)
    if (!hf && helpers) {
        if (lean == 3) QA_LAUNCH_STEP(true, 3, 1);
        else if (lean == 1) QA_LAUNCH_STEP(true, 1, 1);
        else QA_LAUNCH_STEP(true, 0, 1);
        return;
    }
    if (lean == 3) {
        if (hf) QA_LAUNCH_STEP(false, 3, 0);
        else QA_LAUNCH_STEP(true, 3, 0);
    } else if (lean == 1) {
        if (hf) QA_LAUNCH_STEP(false, 1, 0);
        else QA_LAUNCH_STEP(true, 1, 0);
    } else {
        if (hf) QA_LAUNCH_STEP(false, 0, 0);
        else QA_LAUNCH_STEP(true, 0, 0);
    }
#undef QA_LAUNCH_STEP
}

void QA_SCH_FN(launch_physics_step)(bool hf, int blocks, hipStream_t st, const StepArgs &a) {
    if (hf) hipLaunchKernelGGL((qa_env_step_kernel<false, 4, 1, 0, 0, 0, QA_SCH_LEVEL>), dim3(blocks), dim3(QA_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((qa_env_step_kernel<true, 4, 1, 0, 0, 0, QA_SCH_LEVEL>), dim3(blocks), dim3(QA_BLOCK), 0, st, a);
}

void QA_SCH_FN(launch_simulate)(bool hf, int blocks, hipStream_t st, const qa_config &c, const Ptrs &p, const float *torques, const uint8_t *cond) {
    if (hf) hipLaunchKernelGGL((qa_simulate_kernel<false, 4, QA_SCH_LEVEL>), dim3(blocks), dim3(QA_BLOCK), 0, st, c, p, torques, cond);
    else hipLaunchKernelGGL((qa_simulate_kernel<true, 4, QA_SCH_LEVEL>), dim3(blocks), dim3(QA_BLOCK), 0, st, c, p, torques, cond);
}
