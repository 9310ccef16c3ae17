// qa_sim_selfcol_thighs.hip -- the SCH = 2 instantiations of the kernels that run physics (qa_set_self_collision_thighs, include/qa_sim_selfcol.h):
// calf-hip rows and calf-thigh rows.  The same kernel set and the same four launchers as qa_sim_selfcol.hip, named qa_sct_*, in a translation
// unit of their own for the reason given at the top of qa_sim.hip: the kernels of the other two keep the code they had.
#define QA_SCH_LEVEL 2
#define QA_SCH_FN(name) qa_sct_##name
#include "qa_sim_selfcol.hip"
