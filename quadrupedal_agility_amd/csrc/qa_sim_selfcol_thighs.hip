// qa_sim_selfcol_thighs.hip -- self-collision level 2 (qa_set_self_collision_thighs, include/qa_sim_selfcol.h): qa_sim.hip's kernels that run
// physics, instantiated with the calf-hip and the calf-thigh rows (SCH = 2), with their launchers (qa_env_level_sch2) and their copy of the
// constant table, in a translation unit of their own for the reason given at the top of qa_sim.hip.
#define QA_SCH_LEVEL 2
#include "qa_sim.hip"
