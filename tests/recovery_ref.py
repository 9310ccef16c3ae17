"""Host twin of include/qa_sim_reset.h for the tests: a numpy Philox4x32-10 with rng4's counter layout (csrc/qa_device.h), the recovery
pose restated in fp32 from the uniforms, and the contact-set masks with check_termination / _reward_collision restated on them.
Nothing here is float64: every product and sum is rounded to fp32 on its own, as torch writes `(hi - lo) * u + lo`.
"""
import numpy as np

RS_RESET, RS_RECOVERY = 12, 14
SHARED_ENV_WORD = 0xFFFFFFFF                      # the decision's env word: no global env id
BITS = {"base": 1, "hip": 2, "thigh": 4, "calf": 8, "foot": 16}
BODY_NAMES = ["base", "Head_upper", "Head_lower"] + [f"{l}_{p}" for l in ("FL", "FR", "RL", "RR") for p in ("hip", "thigh", "calf", "foot")]
F32 = np.float32
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key):
    """Philox4x32-10: `counter` (..., 4) and `key` (..., 2) of uint32 words -> (..., 4) uint32"""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    lo32, m = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> m) ^ c[1] ^ k0, p1 & lo32, (p0 >> m) ^ c[3] ^ k1, p0 & lo32]
        k0, k1 = (k0 + np.uint64(_W0)) & lo32, (k1 + np.uint64(_W1)) & lo32
    return np.stack(c, axis=-1).astype(np.uint32)


def rng4(seed, env, step, stream, block):
    """rng4 of csrc/qa_device.h: counter (env, step low, stream * 256 + block, step high), key = seed, value (x >> 8) * 2^-24.
    `env`, `step` and `block` broadcast against each other; returns (..., 4) float32."""
    env, step, block = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(step, np.uint64), np.asarray(block, np.uint64))
    ctr = np.stack([env & np.uint64(0xFFFFFFFF), step & np.uint64(0xFFFFFFFF), np.uint64(stream * 256) + block, step >> np.uint64(32)], axis=-1)
    x = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (x >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)


def decision_uniform(seed, steps):
    """the one number a step's recovery decision compares with the probability, for each of `steps`"""
    return rng4(seed, SHARED_ENV_WORD, steps, RS_RECOVERY, 0)[..., 0]


def recovery_steps(seed, steps, prob):
    return decision_uniform(seed, steps) < F32(prob) if prob > 0 else np.zeros(np.shape(steps), bool)


def recovery_uniforms(seed, global_env_ids, step):
    """the 33 uniforms of each env: blocks 1..9 of stream RS_RECOVERY -> (n, 33)"""
    ids = np.asarray(global_env_ids)
    u = rng4(seed, ids[:, None], step, RS_RECOVERY, np.arange(1, 10)[None, :])          # (n, 9, 4)
    return u.reshape(len(ids), 36)[:, :33]


def recovery_pose(u, default_dof_pos, init_pos, origins):
    """(n, 33) uniforms -> root_states (n, 13), dof_pos (n, 12), dof_vel (n, 12), all fp32, in the reference's call order"""
    u = np.asarray(u, F32)
    dof_pos = np.asarray(default_dof_pos, F32)[None, :] * (F32(1.5) * u[:, 0:12] + F32(0.5))
    dof_vel = F32(2.0) * u[:, 12:24] - F32(1.0)
    root = np.zeros((len(u), 13), F32)
    root[:, 0:3] = np.asarray(init_pos, F32)[None, :] + np.asarray(origins, F32)
    root[:, 7:13] = u[:, 24:30] - F32(0.5)
    ang = F32(6.28) * u[:, 30:33] - F32(3.14)
    half = ang * F32(0.5)
    (sr, sp, sy), (cr, cp, cy) = np.sin(half).T.astype(F32), np.cos(half).T.astype(F32)
    root[:, 3] = cy * sr * cp - sy * cr * sp
    root[:, 4] = cy * cr * sp + sy * sr * cp
    root[:, 5] = sy * cr * cp - cy * sr * sp
    root[:, 6] = cy * cr * cp + sy * sr * sp
    return root, dof_pos.astype(F32), dof_vel.astype(F32)


def class_mask(names):
    """the reference's substring rule over the Go2's body names, as a mask of the five body classes; a Head body or no body is refused"""
    mask = 0
    for name in names:
        hit = [b for b in BODY_NAMES if name in b]
        if not hit or any(b.startswith("Head") for b in hit):
            raise NotImplementedError(name)
        for cls, bit in BITS.items():
            if any(b == cls or b.endswith("_" + cls) for b in hit):
                mask |= bit
    return mask


def class_rows(mask):
    """rows of CONTACT_FORCES (N, 19, 3) a mask selects"""
    return [i for i, b in enumerate(BODY_NAMES) for cls, bit in BITS.items() if mask & bit and (b == cls or b.endswith("_" + cls))]


def termination_and_collision(contact_forces, term_mask, pen_mask):
    """check_termination's contact flag (any selected body with |f| > 1) and _reward_collision's count (selected bodies with |f| > 0.1)"""
    norm = np.sqrt((np.asarray(contact_forces, F32) ** 2).sum(-1, dtype=F32))
    return (norm[:, class_rows(term_mask)] > 1.0).any(1), (norm[:, class_rows(pen_mask)] > 0.1).sum(1)
