"""Thin torch-side owner of the device arena behind include/qa_sim.h.

torch is plumbing here: it allocates the slab (so the caching allocator accounts for it),
provides the stream, and exposes zero-copy views of the engine's tensors -- the same role
`gymtorch.wrap_tensor` plays in the reference (legged_robot.py:757-770).
"""
import ctypes as C

import torch

from . import _capi, _cdecl

_TORCH_DT = {_capi.DTYPE_F32: torch.float32, _capi.DTYPE_I64: torch.int64, _capi.DTYPE_U8: torch.uint8,
             _capi.DTYPE_I32: torch.int32, _capi.DTYPE_I16: torch.int16, _capi.DTYPE_F64: torch.float64}
_ITEM = {_capi.DTYPE_F32: 4, _capi.DTYPE_I64: 8, _capi.DTYPE_U8: 1, _capi.DTYPE_I32: 4, _capi.DTYPE_I16: 2, _capi.DTYPE_F64: 8}


class QaSim:
    """One handle = one set of envs on one GPU."""

    def __init__(self, qcfg, device="cuda:0"):
        self.api = _capi.Api(_capi.load_library())          # raises if the HIP library is missing; bound to the library loaded NOW (tools load two builds in one process)
        self.lib = self.api.lib
        if not torch.cuda.is_available():
            raise RuntimeError("quadrupedal_agility_amd needs a ROCm GPU; there is no CPU path")
        self.cfg = qcfg
        self.device = torch.device(device)
        nbytes = self.lib.qa_arena_bytes(C.byref(qcfg))
        if nbytes <= 0:
            raise RuntimeError(f"qa_arena_bytes -> {nbytes}")
        with torch.cuda.device(self.device):
            # over-allocate so that the base can be rounded up to 256 B whatever the allocator returns
            self._slab = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
            shift = (-self._slab.data_ptr()) % 256
            self.arena = self._slab[shift:shift + nbytes]
            h = C.c_void_p()
            self.api.call("create", C.byref(qcfg), self.arena.data_ptr(), nbytes, self.api.stream(self.device), C.byref(h))
        self.h = h
        self.t = {}
        for name, idx in _capi.T.items():
            off, shape, dt = _capi.tensor_info(self.lib, "qa_", qcfg, idx)
            n = 1
            for s in shape:
                n *= s
            self.t[name] = self.arena[off:off + n * _ITEM[dt]].view(_TORCH_DT[dt]).view(*shape)
        self._gae_scratch = torch.zeros(4096, dtype=torch.uint8, device=self.device)
        self.global_step = 0
        # include/qa_sim_reset.h: what the handle does until the setters below are called
        self.recovery_init_prob = 0.0
        self.contact_sets = (_capi.DEFAULT_TERMINATION_MASK, _capi.DEFAULT_PENALISED_MASK)
        self.actuators = None            # include/qa_sim_actuators.h: the P law from cfg.kp / cfg.kd until set_actuators is called

    def reset_all(self):
        self.api.launch("reset_all", self.h, self.global_step, on=self.device)

    def step(self, actions, delay=0):
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert actions.shape == (self.cfg.num_envs, 12)
        self.api.launch("env_step", self.h, actions.data_ptr(), int(delay), self.global_step, on=self.device)
        self.global_step += 1

    def set_lean_exports(self, mask):
        """qa_set_lean_exports: 0 = every tensor refreshed each step (default), 1 = seam-1 / logging exports skipped + two-slot action ring,
        3 = discriminator observations skipped too (training without AMP)"""
        self.api.call("set_lean_exports", self.h, int(mask))
        self.lean_exports = int(mask)

    def set_terrain_curriculum(self, terrain_levels, terrain_types, terrain_origins, env_length, max_episode_length_s):
        """qa_set_terrain_curriculum (include/qa_sim_curriculum.h): from now on the step's reset path moves resetting envs between the rows
        of `terrain_origins` (rows, cols, 3), rewriting `terrain_levels` (N) int64 and ENV_ORIGINS in place.  The handle keeps the POINTERS
        (and this object the tensors, so that they stay alive): call it before a rollout is recorded.  Three Nones switch it off."""
        if terrain_levels is None and terrain_types is None and terrain_origins is None:
            self.api.call("set_terrain_curriculum", self.h, None, None, None, 0, 0, 0.0, 0.0)
            self._curriculum = None
            return
        n = self.cfg.num_envs
        for x, dt, shape in ((terrain_levels, torch.int64, (n,)), (terrain_types, torch.int64, (n,))):
            assert x.is_cuda and x.dtype == dt and x.is_contiguous() and tuple(x.shape) == shape
        o = terrain_origins
        assert o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.dim() == 3 and o.shape[2] == 3
        self.api.call("set_terrain_curriculum", self.h, terrain_levels.data_ptr(), terrain_types.data_ptr(), o.data_ptr(), int(o.shape[0]), int(o.shape[1]),
                      float(env_length), float(max_episode_length_s))
        self._curriculum = (terrain_levels, terrain_types, terrain_origins)

    def set_extra_rewards(self, extra):
        """qa_set_extra_rewards (include/qa_sim_rewards.h): `extra` is cfg_to_c.make_extra_rewards' descriptor; None switches the terms off.
        Allocates the caller-owned buffers -- `extra_episode_sums` (10, N), `feet_air_time` (N, 4), `extra_episode_stats` (2, 16) -- and keeps
        them alive; the handle keeps their POINTERS, so call this before a rollout is recorded."""
        if extra is None:
            self.api.call("set_extra_rewards", self.h, None)
            self.extra_rewards = None
            self.extra_episode_sums = self.feet_air_time = self.extra_episode_stats = self._scan_offsets = None
            return
        n, dev = self.cfg.num_envs, self.device
        self.extra_episode_sums = torch.zeros(_capi.NUM_EXTRA_REWARDS, n, device=dev)
        self.feet_air_time = torch.zeros(n, 4, device=dev)
        self.extra_episode_stats = torch.zeros(2, 16, device=dev)
        self._scan_offsets = None
        if extra.scan_offsets is not None and len(extra.scan_offsets):
            self._scan_offsets = torch.as_tensor(extra.scan_offsets, dtype=torch.float32).reshape(-1, 2).contiguous().to(dev)
        x = _capi.QaExtraRewards()
        for i, v in enumerate(extra.scale_dt):
            x.scale_dt[i] = float(v)
        x.base_height_target, x.max_contact_force, x.step_dt = extra.base_height_target, extra.max_contact_force, extra.step_dt
        x.num_scan_points = 0 if self._scan_offsets is None else int(self._scan_offsets.shape[0])
        x.scan_offsets = None if self._scan_offsets is None else self._scan_offsets.data_ptr()
        x.extra_episode_sums, x.feet_air_time, x.extra_episode_stats = (self.extra_episode_sums.data_ptr(), self.feet_air_time.data_ptr(),
                                                                         self.extra_episode_stats.data_ptr())
        self.api.call("set_extra_rewards", self.h, C.byref(x))
        self.extra_rewards = extra

    def set_self_collision_hips(self, on):
        """qa_set_self_collision_hips (include/qa_sim_selfcol.h): every kernel that runs physics also collides each front calf with the rear hip
        of its side; the force lands on CONTACT_FORCES' calf and HIP rows (a hip force > 1 N ends the episode).  Needs cfg.self_collision;
        it selects other kernels at launch time, so call it before a rollout is recorded."""
        self.api.call("set_self_collision_hips", self.h, int(bool(on)))
        self.self_collision_hips = bool(on)
        self.self_collision_thighs = False                 # the C side drops the calf-thigh rows with the level it sets

    def set_self_collision_thighs(self, on):
        """qa_set_self_collision_thighs (include/qa_sim_selfcol.h): on top of the calf-hip rows, each calf of a front / rear pair of legs collides
        with the other leg's thigh; the force lands on CONTACT_FORCES' calf and THIGH rows (the collision penalty counts it, no termination).
        Switching it on switches the calf-hip rows on too; switching it off leaves them on.  Call it before a rollout is recorded."""
        self.api.call("set_self_collision_thighs", self.h, int(bool(on)))
        self.self_collision_thighs = bool(on)
        if on:
            self.self_collision_hips = True

    def set_recovery_init(self, prob):
        """qa_set_recovery_init (include/qa_sim_reset.h): on a step whose one Philox draw falls below `prob`, every env that resets is thrown
        in tumbled (random roll / pitch / yaw, joints at default x U(0.5, 2), random velocities) instead of taking the handle's reset path.
        0 switches it off.  The value travels in the launch arguments, so call this before a rollout is recorded."""
        self.api.call("set_recovery_init", self.h, float(prob))
        self.recovery_init_prob = float(prob)

    def set_contact_sets(self, termination, penalised):
        """qa_set_contact_sets (include/qa_sim_reset.h): the body classes (masks of _capi.BODY_CLASS_BITS) whose contact ends the episode /
        counts for the collision penalty.  The kernels' defaults are base | hip and thigh | calf.  Call it before a rollout is recorded."""
        self.api.call("set_contact_sets", self.h, int(termination), int(penalised))
        self.contact_sets = (int(termination), int(penalised))

    def set_actuators(self, actuators):
        """qa_set_actuators (include/qa_sim_actuators.h): `actuators` is cfg_to_c.make_actuators' descriptor (control_type 'P' / 'V' / 'T', twelve
        kp, twelve kd); None switches back to the kernels that read cfg.kp / cfg.kd.  The handle copies the gains to a device table of its own
        (the C side allocates it once and frees it with the handle; nothing here has to stay alive).  It selects other kernel instantiations at
        launch time, so call it before a rollout is recorded; refused while a self-collision level is on."""
        if actuators is None:
            self.api.call("set_actuators", self.h, None)
            self.actuators = None
            return
        x = _cdecl.struct("qa_actuators")()
        x.control_type = _cdecl.consts["QA_ACTUATOR_" + actuators.control_type]
        for j in range(_capi.NUM_DOF):
            x.kp[j], x.kd[j] = float(actuators.kp[j]), float(actuators.kd[j])
        with torch.cuda.device(self.device):
            self.api.call("set_actuators", self.h, C.byref(x))
        self.actuators = actuators

    def step_dev(self, actions, delay, step_counter):
        """qa_env_step_dev: the step counter lives in device memory (graph-replayable)."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert step_counter.is_cuda and step_counter.dtype == torch.int64
        self.api.launch("env_step_dev", self.h, actions.data_ptr(), int(delay), step_counter.data_ptr(), on=self.device)

    def physics_step(self, actions, delay=0):
        """qa_env_physics_step: the step without post_physics_step (the task-level env brings its own)"""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous() and actions.shape == (self.cfg.num_envs, 12)
        self.api.launch("env_physics_step", self.h, actions.data_ptr(), int(delay), on=self.device)

    def tsc_reset(self, flags, start_xy, start_yaw, yaw_range, x_range, y_range, pitch_range, step):
        """`step`: the draws' key -- an int, or a 1-element int64 device tensor read when the launch executes (recorded rollouts)"""
        assert flags.is_cuda and flags.dtype == torch.uint8 and start_xy.is_contiguous() and start_yaw.is_contiguous()
        if torch.is_tensor(step):
            assert step.is_cuda and step.dtype == torch.int64
            return self.api.launch("tsc_reset_dev", self.h, flags.data_ptr(), start_xy.data_ptr(), start_yaw.data_ptr(), float(yaw_range), float(x_range),
                                   float(y_range), float(pitch_range), step.data_ptr(), on=self.device)
        self.api.launch("tsc_reset", self.h, flags.data_ptr(), start_xy.data_ptr(), start_yaw.data_ptr(), float(yaw_range), float(x_range),
                        float(y_range), float(pitch_range), int(step), on=self.device)

    def simulate_if(self, torques, cond):
        """one more substep for every env iff the device byte `cond` is non-zero; torques None = the ones applied last"""
        assert cond.is_cuda and cond.dtype == torch.uint8
        self.api.launch("simulate_if", self.h, torques.data_ptr() if torques is not None else None, cond.data_ptr(), on=self.device)

    def simulate(self, torques):
        assert torques.is_cuda and torques.dtype == torch.float32 and torques.is_contiguous()
        self.api.launch("simulate", self.h, torques.data_ptr(), on=self.device)

    def set_mocap(self, frames, clips, first_clip):
        """qa_set_mocap: frames (F,37) fp32, clip table (C,8) float64, clip ranges per gait (MotionLoader.reset_clip_table)"""
        import numpy as np
        f = np.ascontiguousarray(frames, dtype=np.float32)
        ct = np.ascontiguousarray(clips, dtype=np.float64)
        assert f.ndim == 2 and f.shape[1] == _capi.MOCAP_FRAME and ct.ndim == 2 and ct.shape[1] == _capi.MOCAP_CLIP
        first = (C.c_int32 * (_capi.NUM_GAITS + 1))(*[int(x) for x in first_clip])
        self.api.launch("set_mocap", self.h, f.ctypes.data, f.shape[0], ct.ctypes.data, ct.shape[0], first, on=self.device)
        torch.cuda.current_stream(self.device).synchronize()   # host buffers must outlive the async copies

    def debug_post_physics(self, step):
        """qa_debug_post_physics: post_physics_step alone on the arena's state (verification entry)"""
        self.api.launch("debug_post_physics", self.h, int(step), on=self.device)

    def gae(self, rewards, values, dones, last_values, returns, advantages, gamma, lam, normalize=True):
        T, N = rewards.shape[0], rewards.shape[1]
        for x in (rewards, values, dones, last_values, returns, advantages):
            assert x.is_cuda and x.is_contiguous()
        assert dones.dtype == torch.uint8
        self.api.launch("gae", rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), last_values.data_ptr(), returns.data_ptr(), advantages.data_ptr(),
                        T, N, float(gamma), float(lam), int(bool(normalize)), self._gae_scratch.data_ptr(), on=self.device)

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.qa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
