/* qa_sim_curriculum.h -- extension of include/qa_sim.h: the terrain curriculum of the height-field course.
 *
 * Kept apart from qa_sim.h on purpose: that header is the ABI the CPU oracle twins symbol by symbol (tests/test_abi.py), and
 * the curriculum adds neither an arena tensor nor a config field to it.  The library exports this entry point next to the ABI;
 * the Python side binds it through its own list (_capi.EXTENSION_SYMBOLS), not through ABI_SYMBOLS.
 */
#ifndef QA_SIM_CURRICULUM_H
#define QA_SIM_CURRICULUM_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LeggedRobot._update_terrain_curriculum (bbc/legged_gym/envs/base/legged_robot.py:689-711) as reset_idx calls it (:190-192),
 * inside the reset path of the fused step (qa_env_step / qa_env_step_dev) and of qa_debug_post_physics, on height-field handles.
 * For every env that resets in a step, BEFORE its commands are resampled and its state is re-drawn:
 *     d         = |ROOT_STATES[env].xy - ENV_ORIGINS[env].xy|
 *     move_up   = d > env_length / 2
 *     move_down = d < |COMMANDS[env, 0:2]| * max_episode_length_s * 0.5  and not move_up
 *     level     = terrain_levels[env] + move_up - move_down
 *     level     = level >= rows ? a uniform draw from [0, rows) : max(level, 0)
 *     terrain_levels[env] = level;   ENV_ORIGINS[env] = terrain_origins[level, terrain_types[env]]
 * and the env spawns at the new origin in the same launch.  The draw for envs that solve the last row (torch.randint_like in
 * the reference, :707-709) comes from the handle's Philox stream keyed by (seed; env_id_offset + env, step), stream 13.
 * qa_create and qa_reset_all do not apply it (the reference's `init_done` guard, :696-698).
 *
 * terrain_levels (N) int64 is read and written; terrain_types (N) int64 and terrain_origins (rows, cols, 3) fp32 are read
 * (a type outside [0, cols) is clamped; a level outside [0, rows) is repaired by the update itself: floored at 0, or redrawn).  All three are device buffers OWNED BY THE CALLER, contiguous, alive for as long as the
 * handle steps with them: the handle keeps only the pointers, and they travel in the launch arguments of the step.  A recorded
 * rollout (hipGraph) therefore bakes them in: call this BEFORE the first recording, and record again after changing them.
 * Three NULL pointers switch the curriculum off again (rows, cols and the lengths are then ignored).
 * Returns QA_E_ARG on a plane handle (terrain_type != 1), on a mix of NULL and non-NULL pointers and on rows or cols <= 0. */
int qa_set_terrain_curriculum(qa_sim *sim, int64_t *terrain_levels /* (N) device, read + written */,
                              const int64_t *terrain_types /* (N) device */,
                              const float *terrain_origins /* (rows, cols, 3) device */,
                              int32_t rows, int32_t cols, float env_length, float max_episode_length_s);

#ifdef __cplusplus
}
#endif
#endif
