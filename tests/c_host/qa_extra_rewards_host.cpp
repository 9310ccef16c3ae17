// Host twin of the extra reward terms (include/qa_sim_rewards.h): the SAME inline functions post_physics_phase (qa_sim.hip) calls --
// quadrupedal_agility_amd/csrc/qa_rewards.h -- driven from plain C++ on arrays, so that tests/test_extra_rewards_cpu.py checks the
// arithmetic and the summation order against the reference's outputs (tests/golden/extra_rewards.npz) without a GPU.
// Built by that test as a shared library: c++ -O2 -std=c++17 -shared -fPIC.  Row-major arrays; per-term arrays are (terms, n).
#include <stdint.h>

#include "../../quadrupedal_agility_amd/csrc/qa_rewards.h"

extern "C" int qa_extra_rewards_host(int n, int num_scan, const float *base_lin_vel /* (n,3) */, const float *base_ang_vel /* (n,3) */,
                                     const float *projected_gravity /* (n,3) */, const float *root_z /* (n) */, const float *measured_heights /* (n,num_scan) */,
                                     const float *dof_pos /* (n,12) */, const float *dof_vel /* (n,12) */, const float *default_dof_pos /* (12) */,
                                     const float *foot_force /* (n,4,3) */, const float *commands /* (n,5) */, const int64_t *reset /* (n) */,
                                     const uint8_t *time_out /* (n) */, const float *base_terms /* (14,n) */, const float *base_scale_dt /* (14) */,
                                     const qa_extra_rewards *x, int only_positive, float *feet_air_time /* (n,4) in/out */, uint8_t *last_contacts /* (n,4) in/out */,
                                     float *base_sums /* (14,n) in/out */, float *extra_sums /* (10,n) in/out */, float *extra_terms /* (10,n) out */, float *rew /* (n) out */) {
    if (n <= 0 || !x) return -1;
    for (int e = 0; e < n; ++e) {
        float xt[QA_NUM_EXTRA_REWARDS], bt[QA_NUM_REWARDS], bs[QA_NUM_REWARDS], xs[QA_NUM_EXTRA_REWARDS];
        xt[QA_XR_ANG_VEL_XY] = qa_rw_ang_vel_xy(base_ang_vel[3 * e], base_ang_vel[3 * e + 1]);
        float mean_h = root_z[e];
        if (num_scan > 0) {
            float s = 0.f;
            for (int i = 0; i < num_scan; ++i) s += root_z[e] - measured_heights[(int64_t)e * num_scan + i];
            mean_h = s / (float)num_scan;
        }
        xt[QA_XR_BASE_HEIGHT] = qa_rw_base_height(mean_h, x->base_height_target);
        const float cnorm = qa_rw_command_norm(commands[5 * e], commands[5 * e + 1]);
        float dv = 0.f, air = 0.f, still = 0.f, over = 0.f; int stumble = 0;
        const bool air_on = x->scale_dt[QA_XR_FEET_AIR_TIME] != 0.0f;
        for (int leg = 0; leg < 4; ++leg) {
            const float *q = dof_pos + 12 * e + 3 * leg, *qd = dof_vel + 12 * e + 3 * leg, *q0 = default_dof_pos + 3 * leg, *f = foot_force + 12 * e + 3 * leg;
            dv += qa_rw_dof_vel_leg(qd[0], qd[1], qd[2]);
            if (air_on) {
                const bool contact_z = f[2] > 1.0f, contact = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) > 2.0f;
                air += qa_rw_feet_air_time_leg(&feet_air_time[4 * e + leg], contact_z, contact, x->step_dt);
                last_contacts[4 * e + leg] = contact_z;
            }
            stumble |= qa_rw_feet_stumble_leg(f[0], f[1], f[2]);
            still += qa_rw_stand_still_leg(q[0], q[1], q[2], q0[0], q0[1], q0[2]);
            over += qa_rw_feet_contact_forces_leg(f[0], f[1], f[2], x->max_contact_force);
        }
        xt[QA_XR_DOF_VEL] = dv;
        xt[QA_XR_FEET_AIR_TIME] = air * qa_rw_moving(cnorm);
        xt[QA_XR_FEET_CONTACT_FORCES] = over;
        xt[QA_XR_FEET_STUMBLE] = stumble ? 1.0f : 0.0f;
        xt[QA_XR_LIN_VEL_Z] = qa_rw_lin_vel_z(base_lin_vel[3 * e + 2]);
        xt[QA_XR_ORIENTATION] = qa_rw_orientation(projected_gravity[3 * e], projected_gravity[3 * e + 1]);
        xt[QA_XR_STAND_STILL] = still * qa_rw_standing(cnorm);
        xt[QA_XR_TERMINATION] = qa_rw_termination(reset[e] != 0, time_out[e] != 0);
        for (int r = 0; r < QA_NUM_REWARDS; ++r) { bt[r] = base_terms[(int64_t)r * n + e]; bs[r] = base_sums[(int64_t)r * n + e]; }
        for (int r = 0; r < QA_NUM_EXTRA_REWARDS; ++r) xs[r] = extra_sums[(int64_t)r * n + e];
        rew[e] = qa_rw_total(bt, base_scale_dt, bs, xt, x->scale_dt, xs, only_positive);
        if (reset[e]) {          // reset_idx :224, :231-234
            for (int r = 0; r < QA_NUM_REWARDS; ++r) bs[r] = 0.f;
            for (int r = 0; r < QA_NUM_EXTRA_REWARDS; ++r) xs[r] = 0.f;
            for (int leg = 0; leg < 4; ++leg) feet_air_time[4 * e + leg] = 0.f;
        }
        for (int r = 0; r < QA_NUM_REWARDS; ++r) base_sums[(int64_t)r * n + e] = bs[r];
        for (int r = 0; r < QA_NUM_EXTRA_REWARDS; ++r) { extra_sums[(int64_t)r * n + e] = xs[r]; extra_terms[(int64_t)r * n + e] = xt[r]; }
    }
    return 0;
}
