"""The obstacle curriculum of the agility course: `LeggedRobot._update_obstacle_curriculum` of the reference
(tsc/legged_gym/envs/base/legged_robot.py:917-957, called from reset_idx at :361) without its deep copy and re-upload of the whole map.

The reference rebuilds the height map and the goals from the as-built course plus a bias that grows by `curr_step` per raise.  Only the
cells under `bar_jump_mask` / `tire_jump_mask` and the goal entries under the two goal masks ever change, so this module lists them once
(`compact_lists`: a few hundred cells per env against 28,000 in the map), tabulates the reference's float64 arithmetic per count on the
host (`increment_tables`), and leaves the per-step work to one launch (`qa_tsc_obstacle_curriculum`, include/qa_tsc_curriculum.h) or to
its restatement in torch (`ObstacleCurriculum.update_torch`: the path of QA_TSC_GLUE=0 and of a CPU backend, and what the kernel is
tested against).  Both decide on the device, from the step counter's twin, a success-rate scalar and the step's any_reset byte."""
import ctypes as C

import numpy as np
import torch

from quadrupedal_agility_amd import _capi
from quadrupedal_agility_amd.tsc.legged_gym.utils.obstacle import NO_CEILING

BAR, TYRE = _capi.TSC_OBST_BAR, _capi.TSC_OBST_TYRE


def increment_tables(curr_step, vertical_scale, bar_jump_max_range, tire_jump_max_range):
    """-> (increments (L, 2) int32, biases (L, 2) float64) for count = 0 .. L - 1, columns (bar, tyre), spelled as the reference spells them:
    bias = min(count * curr_step, max_range[1] - max_range[0]) (:930-934), increment = int(bias / vertical_scale) (:941-942), Python floats.
    L - 1 is one past the first count at which both biases sit on their caps: from there on every count gives the last row."""
    caps = (bar_jump_max_range[1] - bar_jump_max_range[0], tire_jump_max_range[1] - tire_jump_max_range[0])
    if not curr_step > 0:
        raise ValueError("obstacle.curr_step must be positive")
    at_cap = 0
    while any(at_cap * curr_step < cap for cap in caps):
        at_cap += 1
    inc, bias = [], []
    for count in range(at_cap + 2):
        b = [min(count * curr_step, cap) for cap in caps]
        bias.append(b)
        inc.append([int(x / vertical_scale) for x in b])
    return np.asarray(inc, dtype=np.int32), np.asarray(bias, dtype=np.float64)


def compact_lists(obstacle):
    """What a raise touches, from the generator's masks: height cells (flat index into the map, kind, as-built sample), the tyre's cells of
    the ceiling field, and the masked entries of the flat (N, slots, 3) goals tensor of `Obstacle.flat_goals()`, repeats of the last goal included."""
    ob = obstacle
    cells = ob.height_field_raw.size
    if cells >= 2 ** 31:
        raise ValueError("the course map has more cells than an int32 index reaches")
    raw = ob.height_field_raw.reshape(-1)
    ib, it = np.flatnonzero(ob.bar_jump_mask.reshape(-1)), np.flatnonzero(ob.tire_jump_mask.reshape(-1))
    cell_index = np.concatenate([ib, it])
    cell_kind = np.concatenate([np.full(len(ib), BAR, np.uint8), np.full(len(it), TYRE, np.uint8)])
    order = np.argsort(cell_index, kind="stable")
    cell_index, cell_kind = cell_index[order], cell_kind[order]
    ic = np.flatnonzero((ob.tire_ceiling_mask & (ob.ceiling_raw != NO_CEILING)).reshape(-1))
    # goals: (N, K, G, 3) -> slot k * G + g of (N, K * G + repeat, 3)
    n, k, g, _ = ob.env_goals.shape
    slots = k * g + ob.last_goal_repeat
    gi, gk, gb = [], [], []
    for kind, mask in ((BAR, ob.bar_jump_goal_mask), (TYRE, ob.tire_jump_goal_mask)):
        for e, j, m, c in zip(*np.nonzero(mask)):
            slot = j * g + m
            copies = [slot]
            if slot == k * g - 1:                  # the last goal: its repeats are copies made AFTER the bias is added (:951-957)
                if c == 1 and ob.last_goal_repeat:
                    raise NotImplementedError("a masked y coordinate of the last goal: its repeats add 0.1 (k + 1) in fp32 after the bias")
                copies += [k * g + r for r in range(ob.last_goal_repeat)]
            for s in copies:
                gi.append((e * slots + s) * 3 + c); gk.append(kind); gb.append(ob.env_goals[e, j, m, c])
    gi = np.asarray(gi, dtype=np.int64)
    order = np.argsort(gi, kind="stable")
    return dict(cell_index=cell_index.astype(np.int32), cell_kind=cell_kind, cell_base=raw[cell_index].astype(np.int16),
                ceiling_index=ic.astype(np.int32), ceiling_base=ob.ceiling_raw.reshape(-1)[ic].astype(np.int16),
                goal_index=gi[order].astype(np.int32), goal_kind=np.asarray(gk, dtype=np.uint8)[order], goal_base=np.asarray(gb, dtype=np.float64)[order],
                map_cells=int(cells), goal_floats=int(n * slots * 3))


class ObstacleCurriculum:
    """Device side of the curriculum of one env: lists, tables, the state record [count, bar bias, tyre bias (float64 bits), global_counter of the
    last raise], the success-rate scalar and the offset that turns common_step_counter's device twin into global_counter."""

    def __init__(self, lists, tables, threshold, period, device):
        dev = self.device = torch.device(device)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
        self.lists = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in lists.items()}
        self.increments, self.biases = T(tables[0]), T(tables[1])
        self.last = int(self.increments.shape[0]) - 1
        self.threshold, self.period = float(threshold), int(period)
        if self.period <= 0:
            raise ValueError("the curriculum's period (2 * max_episode_length) must be positive")
        self.state = torch.tensor([0, 0, 0, -1], dtype=torch.int64, device=dev)
        self.rate = torch.zeros(1, dtype=torch.float64, device=dev)
        self.offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self._offset_host = 0
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._long = {k: self.lists[k].long() for k in ("cell_index", "cell_kind", "ceiling_index", "goal_index", "goal_kind")}
        self.maps, self.ceiling, self.goals, self._args = [], None, None, None

    @classmethod
    def from_course(cls, obstacle, period, device):
        c = obstacle.cfg
        tables = increment_tables(c.curr_step, obstacle.vertical_scale, c.bar_jump_max_range, c.tire_jump_max_range)
        return cls(compact_lists(obstacle), tables, c.curr_threshold, period, device)

    def bind(self, height_samples, scan_samples, ceiling_samples, env_goals):
        """the tensors that hold the course (the scan's map may be the engine's own, or None)"""
        L = self.lists
        maps = [height_samples]
        if scan_samples is not None and scan_samples.data_ptr() != height_samples.data_ptr():
            maps.append(scan_samples)
        for m in maps + [ceiling_samples]:
            if m.dtype != torch.int16 or not m.is_contiguous() or m.numel() != L["map_cells"]:
                raise ValueError("the course maps are contiguous int16 tensors of the generator's size")
        if env_goals.dtype != torch.float32 or not env_goals.is_contiguous() or env_goals.numel() != L["goal_floats"]:
            raise ValueError("env_goals is the contiguous fp32 (N, slots, 3) tensor of Obstacle.flat_goals()")
        self.maps, self.ceiling, self.goals, self._args = maps, ceiling_samples, env_goals, None

    # ---- host <-> device scalars (between replays, never inside a recording)
    def set_rate(self, value):
        self.rate.fill_(float(value))

    def set_offset(self, value):
        if int(value) != self._offset_host:
            self._offset_host = int(value)
            self.offset.fill_(int(value))

    def read_state(self):
        """-> (count, bar_jump_bias, tire_jump_bias, global_counter of the last raise); a host read"""
        s = self.state.cpu()
        b = s[1:3].view(torch.float64)
        return int(s[0]), float(b[0]), float(b[1]), int(s[3])

    # ---- the update
    def launch(self, lib, step_dev, any_reset, stream):
        if self._args is None:
            L, a = self.lists, _capi.QaTscObstCurr()
            a.success_rate, a.counter_offset = self.rate.data_ptr(), self.offset.data_ptr()
            a.threshold, a.period, a.state, a.ticket = self.threshold, self.period, self.state.data_ptr(), self.ticket.data_ptr()
            a.increments, a.biases, a.last = self.increments.data_ptr(), self.biases.data_ptr(), self.last
            a.cell_index, a.cell_kind, a.cell_base, a.num_cells = L["cell_index"].data_ptr(), L["cell_kind"].data_ptr(), L["cell_base"].data_ptr(), L["cell_index"].numel()
            a.height_samples, a.scan_samples, a.map_cells = self.maps[0].data_ptr(), self.maps[1].data_ptr() if len(self.maps) > 1 else None, L["map_cells"]
            a.ceiling_index, a.ceiling_base, a.num_ceiling_cells = L["ceiling_index"].data_ptr(), L["ceiling_base"].data_ptr(), L["ceiling_index"].numel()
            a.ceiling_samples = self.ceiling.data_ptr()
            a.goal_index, a.goal_kind, a.goal_base, a.num_goal_entries = L["goal_index"].data_ptr(), L["goal_kind"].data_ptr(), L["goal_base"].data_ptr(), L["goal_index"].numel()
            a.env_goals, a.goal_floats = self.goals.data_ptr(), L["goal_floats"]
            self._args = a
        a = self._args
        a.step_counter, a.any_reset = step_dev.data_ptr(), any_reset.data_ptr()
        _capi.API.check("tsc_obstacle_curriculum", lib.qa_tsc_obstacle_curriculum(C.byref(a), stream))

    def update_torch(self, step_dev, any_reset):
        """the same update as tensor operations on the same lists and tables (no host read, no host branch)"""
        L, I = self.lists, self._long
        gc = step_dev.reshape(-1)[0].to(torch.int64) - self.offset[0]
        trig = (any_reset.reshape(-1)[0] != 0) & (torch.remainder(gc, self.period) == 0) & (self.rate[0] > self.threshold)
        count = self.state[0] + 1
        k = count.clamp(0, self.last)
        inc, bias = self.increments[k], self.biases[k]                       # (2,) int32, (2,) float64
        new_h = (L["cell_base"].to(torch.int32) + inc[I["cell_kind"]]).to(torch.int16)
        for m in self.maps:
            flat = m.view(-1)
            flat[I["cell_index"]] = torch.where(trig, new_h, flat[I["cell_index"]])
        flat = self.ceiling.view(-1)
        flat[I["ceiling_index"]] = torch.where(trig, (L["ceiling_base"].to(torch.int32) + inc[TYRE]).to(torch.int16), flat[I["ceiling_index"]])
        flat = self.goals.view(-1)
        flat[I["goal_index"]] = torch.where(trig, (L["goal_base"] + bias[I["goal_kind"]]).to(torch.float32), flat[I["goal_index"]])
        new = torch.cat([count.reshape(1), bias.view(torch.int64), gc.reshape(1)])
        self.state.copy_(torch.where(trig, new, self.state))
