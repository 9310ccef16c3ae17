// qa_sim_selfcol.hip -- self-collision level 1 (qa_set_self_collision_hips, include/qa_sim_selfcol.h): qa_sim.hip's kernels that run physics,
// instantiated with the calf-hip rows (SCH = 1), with their launchers (qa_env_level_sch1) and their copy of the constant table, in a
// translation unit of their own so that the kernels of the other levels keep the code they had (see the top of qa_sim.hip).
#define QA_SCH_LEVEL 1
#include "qa_sim.hip"
