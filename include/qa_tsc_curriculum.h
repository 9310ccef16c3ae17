/* qa_tsc_curriculum.h -- extension of include/qa_sim.h: the obstacle curriculum of the task-level agility course.
 *
 * A sibling of qa_sim_curriculum.h and kept apart from qa_sim.h for the same reason: no arena tensor, no config field, no oracle
 * twin (the torch restatement in tsc/legged_gym/obstacle_curriculum.py is the twin).  The library exports the entry point next to
 * the ABI; the Python side binds it through _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_TSC_CURRICULUM_H
#define QA_TSC_CURRICULUM_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QA_TSC_OBST_BAR 0
#define QA_TSC_OBST_TYRE 1
/* the state record: int64 count, then the two biases as IEEE doubles, then global_counter of the last raise (-1: none yet) */
#define QA_TSC_OBST_STATE_WORDS 4

/* LeggedRobot._update_obstacle_curriculum (tsc/legged_gym/envs/base/legged_robot.py:917-957) as reset_idx calls it (:361), as ONE
 * launch of the env step between qa_tsc_reset_stats (whose any_reset byte it reads) and qa_tsc_reset_where (which re-gathers the
 * current goals from env_goals).  Every pointer is device memory owned by the caller; nothing is allocated, nothing is read back,
 * the launch geometry depends on the list lengths only: the call can be recorded into a hipGraph and replayed.
 *
 *     global_counter = *step_counter - *counter_offset
 *     raise          = *any_reset != 0  and  global_counter % period == 0  and  *success_rate > threshold
 * When `raise` is false every workgroup returns after these reads.  When it is true:
 *     count = state[0] + 1;   k = min(count, last)
 *     height_samples[cell_index[i]] = cell_base[i] + increments[k][cell_kind[i]]          (and scan_samples, when not NULL)
 *     ceiling_samples[ceiling_index[i]] = ceiling_base[i] + increments[k][QA_TSC_OBST_TYRE]
 *     env_goals[goal_index[i]] = (float)(goal_base[i] + biases[k][goal_kind[i]])          (the sum in double, as the reference's numpy)
 *     state = {count, biases[k][0], biases[k][1], global_counter}
 * Absolute from the as-built values, not cumulative.  `increments` (last + 1, 2) int32 and `biases` (last + 1, 2) double are the
 * host's  int(bias / vertical_scale)  and  min(count * curr_step, max_range[1] - max_range[0])  for count 0 .. last: the float64
 * truncation is the reference's and is not redone on the device.  The count itself is unbounded.
 * The state is written by the last workgroup to finish (a ticket, as qa_tsc_push advances its counter): every workgroup has read
 * the old count by then.  `ticket` is one int32, zero before the first call; the kernel leaves it zero.
 * Indices outside [0, map_cells) / [0, goal_floats) are skipped.  Returns QA_E_ARG on a missing pointer, period <= 0, last < 0. */
typedef struct qa_tsc_obst_curr {
    const int64_t *step_counter;      /* common_step_counter's device twin */
    const int64_t *counter_offset;    /* common_step_counter - global_counter */
    const double *success_rate;
    const uint8_t *any_reset;
    double threshold;
    int64_t period;                   /* 2 * max_episode_length */
    int64_t *state;                   /* [QA_TSC_OBST_STATE_WORDS] */
    int32_t *ticket;
    const int32_t *increments;
    const double *biases;
    int32_t last;
    int32_t reserved;
    const int32_t *cell_index;        /* (num_cells) flat indices into the height maps */
    const uint8_t *cell_kind;         /* (num_cells) QA_TSC_OBST_BAR / _TYRE */
    const int16_t *cell_base;         /* (num_cells) as-built samples */
    int64_t num_cells;
    int16_t *height_samples;          /* the engine's HEIGHT_SAMPLES */
    int16_t *scan_samples;            /* the height scan's map when it is another tensor, else NULL */
    int64_t map_cells;                /* rows * cols of the maps and of the ceiling field */
    const int32_t *ceiling_index;     /* (num_ceiling_cells) the tyre's cells of CEILING_SAMPLES */
    const int16_t *ceiling_base;
    int64_t num_ceiling_cells;
    int16_t *ceiling_samples;         /* may be NULL when num_ceiling_cells == 0 */
    const int32_t *goal_index;        /* (num_goal_entries) flat indices into env_goals (N, slots, 3) */
    const uint8_t *goal_kind;
    const double *goal_base;
    int64_t num_goal_entries;
    float *env_goals;
    int64_t goal_floats;              /* N * slots * 3 */
} qa_tsc_obst_curr;

int qa_tsc_obstacle_curriculum(const qa_tsc_obst_curr *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
