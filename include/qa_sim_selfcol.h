/* qa_sim_selfcol.h -- extension of include/qa_sim.h: each front calf collides with the rear hip of its side inside the physics substep, and
 * (a second switch) each calf of a front / rear pair with the other leg's thigh.
 *
 * Kept apart from qa_sim.h for the reason qa_sim_rewards.h is: that header is the ABI the CPU oracle twins symbol by symbol
 * (tests/test_abi.py), and this feature adds neither an arena tensor nor a config field to it.  The library exports the entry point next to
 * the ABI; the Python side binds it through _capi.EXTENSION_SYMBOLS.
 */
#ifndef QA_SIM_SELFCOL_H
#define QA_SIM_SELFCOL_H

#include "qa_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference enables every self-collision pair of the Go2 (`self_collisions = 0`, bbc/.../go2_locomotion_config.py:72,
 * tsc/.../go2_agility_config.py:43) and ends the episode when a hip carries more than 1 N (`terminate_after_contacts_on = ["base", "hip"]`).
 * cfg.self_collision alone collides the calf capsules of neighbouring legs.  With on != 0 every kernel that runs physics -- qa_env_step /
 * qa_env_step_dev (plane with and without helper wavefronts, height field), qa_env_physics_step, qa_simulate / qa_simulate_if -- also solves
 * one frictionless contact row between the calf capsule of a front leg (knee to foot centre, radius 13 mm growing to 22 mm) and the hip
 * cylinder of the rear leg of the same side taken as a capsule (segment (0, +-0.06, 0) .. (0, +-0.10, 0) of the hip link, radius 46 mm):
 * the one ordered (calf leg, hip leg) relation that can come within the contact offset under the URDF joint limits.
 *   - The row is active while the gap is below cfg.contact_offset, with the calf rows' bias rule (gap / dt, capped at
 *     cfg.max_depenetration_velocity while penetrating).
 *   - CONTACT_FORCES carries the force on the calf body of the front leg (5 + 4 leg) and its opposite on the HIP body of the rear leg
 *     (3 + 4 leg): the termination check, the collision penalty and the task-level masks read it like any other contact force, so a hip
 *     force above 1 N ends the episode on that step.
 *   - on == 0 switches back to the kernels without the row; with it every arena tensor is bit-identical to never having called this.
 *
 * The choice selects other kernel instantiations at launch time and is not part of the launch arguments: a recorded rollout (hipGraph)
 * bakes it in.  Call this BEFORE the first recording, and record again after changing it.
 * Returns QA_E_ARG on a NULL handle and, with on != 0, on a handle created with cfg.self_collision == 0. */
int qa_set_self_collision_hips(qa_sim *sim, int on);

/* The next pair class: a calf against the THIGH of the front / rear neighbour of its side.  The thigh is the URDF's thigh box 0.11 x 0.0245 x 0.034
 * as its circumscribed capsule (segment (0, 0, -0.0515) .. (0, 0, -0.1615) of the thigh link, radius 21 mm).  The joint limits prune none of the
 * twelve ordered (calf leg, thigh leg) relations; the four front / rear relations of the same side get a row -- FL calf on RL thigh, RL calf on
 * FL thigh, FR calf on RR thigh, RR calf on FR thigh -- and the left / right and diagonal relations stay unmodelled.
 *   - One internal level serves both setters: 0 none, 1 calf-hip rows, 2 calf-hip and calf-thigh rows.  qa_set_self_collision_hips(on) sets it
 *     to on ? 1 : 0; this call sets it to 2 with on != 0, and from 2 back to 1 with on == 0 (levels 0 and 1 stay as they are).
 *   - Two more frictionless rows per front / rear pair, with the calf-hip row's activity and bias rules.
 *   - CONTACT_FORCES carries the force on the calf body (5 + 4 leg) and its opposite on the THIGH body (4 + 4 other leg): the collision
 *     penalty and the task-level masks read it; no termination follows from it.
 *   - While no calf-thigh pair is inside the contact offset every arena tensor is bit-identical to level 1.
 * Like the call above it selects kernel instantiations: call it BEFORE the first recording, and record again after changing it.
 * Returns QA_E_ARG on a NULL handle and, with on != 0, on a handle created with cfg.self_collision == 0. */
int qa_set_self_collision_thighs(qa_sim *sim, int on);

#ifdef __cplusplus
}
#endif
#endif
