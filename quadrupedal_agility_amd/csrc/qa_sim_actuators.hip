// qa_sim.hip once more, as the unit of the actuator kernels (qa_set_actuators, include/qa_sim_actuators.h): the step kernels with ACT = 1 at
// self-collision level 0, their own copy of the constant table and their launchers (qa_env_level_act, k_levels[QA_ACT_UNIT] of qa_sim.hip)
#define QA_ACTUATORS 1
#include "qa_sim.hip"
