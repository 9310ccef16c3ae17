"""recording.MinibatchSchedule without a device: what it feeds, in which order it replays, and what a recording contains.  Graphs are stand-ins that
log `replay()`, the gradient collective a stand-in that logs `all_reduce_`.  The permuted copies are filled by a torch `index_select` standing in
for `fused.gather_rows` (one HIP launch, which needs a GPU); everything else is the schedule's own code.  nmb = 3 minibatches of mb = 5 rows over
17-row sources: rows 15 and 16 lie outside the permutation."""
import pytest
import torch

NMB, MB, ROWS, EPOCHS = 3, 5, 17, 2


@pytest.fixture
def sched_mod(monkeypatch):
    from quadrupedal_agility_amd.rsl_rl import recording
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused

    def gather_rows(idx, srcs, dsts=None):
        for s, d in zip(srcs, dsts):
            d.copy_(s.reshape(s.shape[0], -1).index_select(0, idx))
        return dsts
    monkeypatch.setattr(fused, "gather_rows", gather_rows)
    return recording


class _Graph:
    def __init__(self, log, name, snapshot=lambda: None):
        self.log, self.name, self.snapshot = log, name, snapshot

    def replay(self):
        self.log.append(("replay", self.name, self.snapshot()))


class _Sync:
    world = 2

    def __init__(self, log):
        self.log = log

    def all_reduce_(self, t):
        self.log.append(("all_reduce", t))


def _sources():
    g = torch.Generator().manual_seed(3)
    return torch.randn(ROWS, 4, generator=g), torch.randn(ROWS, generator=g), torch.randperm(NMB * MB, generator=g)


def test_index_mode_copies_the_next_slice_before_every_replay(sched_mod):
    src2, src1, perm = _sources()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=False)
    assert s.bufs is None and s.idx.shape == (MB,) and s.idx.dtype == torch.int64 and s.feeds() == [(s.idx,)]
    log = []
    s.append((_Graph(log, "step", lambda: s.idx.clone()), None, None))
    s.run(perm, EPOCHS)
    assert [e[:2] for e in log] == [("replay", "step")] * (EPOCHS * NMB)
    for k, (_, _, idx) in enumerate(log):
        i = k % NMB
        assert torch.equal(idx, perm[i * MB:(i + 1) * MB])


def test_slot_mode_fills_permuted_copies_once_and_never_samples_the_tail(sched_mod):
    src2, src1, perm = _sources()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=True)
    assert s.idx is None and [tuple(b.shape) for b in s.bufs] == [(NMB * MB, 4), (NMB * MB, 1)]      # a 1-D source gets width 1
    log = []
    for i in range(NMB):
        s.append((_Graph(log, i, lambda i=i: [v.clone() for v in s.slot(i)]), None, None))
    s.run(perm, EPOCHS)
    assert [e[1] for e in log] == [0, 1, 2, 0, 1, 2]
    seen = []
    for _, i, (rows2, rows1) in log:          # what each replay read is its slice of the permutation, of both sources
        sl = perm[i * MB:(i + 1) * MB]
        assert torch.equal(rows2, src2[sl]) and torch.equal(rows1.view(-1), src1[sl])
        seen.append(sl)
    assert torch.equal(torch.cat(seen[:NMB]).sort().values, torch.arange(NMB * MB))      # rows 15 and 16 appear in no slot
    for row in (15, 16):
        assert not any(torch.equal(b2, src2[row]) for b2 in s.bufs[0]) and not (s.bufs[1].view(-1) == src1[row]).any()
    views = s.slot(1)
    assert views[0].data_ptr() == s.bufs[0][MB].data_ptr() and views[0].shape == (MB, 4) and views[1].shape == (MB, 1)      # slots are views, not copies


def test_data_parallel_steps_replay_around_the_collective(sched_mod):
    src2, src1, perm = _sources()
    for permuted in (True, False):
        s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=permuted)
        log, sync = [], _Sync([])
        sync.log = log
        buckets = [torch.full((2,), float(i)) for i in range(NMB if permuted else 1)]
        for i, b in enumerate(buckets):
            s.append((_Graph(log, ("a", i)), _Graph(log, ("b", i)), b))
        s.run(perm, EPOCHS, sync)
        steps = [log[k:k + 3] for k in range(0, len(log), 3)]
        assert len(steps) == EPOCHS * NMB
        for k, (a, r, b) in enumerate(steps):
            i = k % NMB if permuted else 0
            assert a[:2] == ("replay", ("a", i)) and r[0] == "all_reduce" and r[1] is buckets[i] and b[:2] == ("replay", ("b", i))


def test_epoch_form_is_one_replay_per_epoch_and_no_index_copy(sched_mod):
    src2, src1, perm = _sources()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=True)
    log = []
    s.append((_Graph(log, "epoch"), None, None))
    s.run(perm, EPOCHS)
    assert [e[:2] for e in log] == [("replay", "epoch")] * EPOCHS and s.idx is None


@pytest.fixture
def fake_capture(monkeypatch):
    """torch.cuda.CUDAGraph / graph / graph_pool_handle stand-ins: a `with` body runs at once, `log` keeps captures"""
    import contextlib
    log = []

    class Graph:
        pass

    @contextlib.contextmanager
    def graph(g, pool=None, stream=None):
        log.append(("capture", pool))
        yield
        log.append(("end",))
    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(torch.cuda, "graph", graph)
    monkeypatch.setattr(torch.cuda, "graph_pool_handle", lambda: "POOL")
    return log


def _step_fns(log, stats_as_tensor):
    def front(*feed):
        log.append(("front", [f.data_ptr() for f in feed]))
        stats = (torch.tensor(1.0), torch.tensor(2.0))
        return torch.tensor(0.5), torch.stack(stats) if stats_as_tensor else stats
    return front, lambda kl: log.append(("apply", float(kl))), lambda: log.append(("zero",))


@pytest.mark.parametrize("stats_as_tensor", [True, False])
def test_recordings_of_the_three_forms_hold_what_the_sites_recorded(sched_mod, fake_capture, stats_as_tensor):
    src2, src1, _ = _sources()
    log = fake_capture
    front, apply, zero = _step_fns(log, stats_as_tensor)
    names = lambda: [e[0] for e in log]
    # one recording per slot: [front, apply, acc += stats] each, gradients dropped after each so that the next creates its own; one pool
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=True)
    acc = torch.zeros(2)
    s.record_steps(front, apply, acc, zero)
    assert names() == ["capture", "front", "apply", "end", "zero"] * NMB and len(s) == NMB and all(gb is None and b is None for _, gb, b in s)
    assert [e[1] for e in log if e[0] == "front"] == [[v.data_ptr() for v in s.slot(i)] for i in range(NMB)]
    assert {e[1] for e in log if e[0] == "capture"} == {"POOL"} and s.acc is acc and torch.equal(acc, torch.tensor([3.0, 6.0]))
    # the slots of an epoch as ONE recording, gradients dropped after each slot INSIDE it
    log.clear()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=True)
    s.record_steps(front, apply, torch.zeros(2), zero, epoch=True)
    assert names() == ["capture"] + ["front", "apply", "zero"] * NMB + ["end"] and len(s) == 1
    # index buffer: one recording fed the buffer itself, nothing zeroed by the schedule
    log.clear()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=False)
    s.record_steps(front, apply, torch.zeros(2))
    assert names() == ["capture", "front", "apply", "end"] and log[1][1] == [s.idx.data_ptr()] and len(s) == 1
    # the data-parallel pair: front in the first graph, apply in the second; the stacked statistics and the bucket stay with the schedule
    log.clear()
    s = sched_mod.MinibatchSchedule(NMB, MB, [src2, src1], permuted=False)
    acc = torch.zeros(2)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    s.record_steps(front, apply, acc, sync=_Sync(log), params=[p])
    assert names() == ["capture", "front", "end", "capture", "apply", "end"] and log[4][1] == 0.25          # the KL mean over 2 ranks
    (ga, gb, bucket), = s
    assert gb is not None and bucket.shape == (4,) and len(s.held) == 1 and s.held[0].shape == (2,) and torch.equal(acc, torch.tensor([1.0, 2.0]))
