"""Recording launches into hipGraphs: the ceremony every recorded path of both trees shares (rollouts, PPO / discriminator / DAgger steps,
the vision student's env step).  What a site records, what it synchronises, zeroes or warms up first, and what it does once a capture has
failed (mark its slot False, run the eager loop) stay at the site.  The PPO and DAgger updates of both learners share more than the ceremony --
how minibatches are fed, which recordings make up an epoch, the `epochs x graphs` replay: MinibatchSchedule.  Its sites keep their sources,
the step itself (`front` / `apply`), the pre-pass and device scalars they fill before a run, their warm-up, the choice of form, the eager fallback."""
import contextlib
import gc
import os
import traceback

import torch


@contextlib.contextmanager
def no_gc():
    """No cyclic garbage collection while a stream is capturing: a collection that happens to run inside the capture can
    destroy old device objects (graphs, tensors with recorded events), whose destructors call HIP APIs that are illegal
    during capture and abort the process.  (torch.cuda.graph collects once on entry; this keeps it from running again.)"""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def record(body, pool=None, stream=None):
    """Run `body()` under capture (its host side effects happen now, its GPU work on replay).  Returns (graph, what body returned)."""
    g = torch.cuda.CUDAGraph()
    with no_gc(), torch.cuda.graph(g, pool=pool, stream=stream):
        out = body()
    return g, out


def capture_failed(tag, e):
    """A capture is never fatal, the eager launches are the same arithmetic: say so (QA_DEBUG_GRAPH=1: with the traceback) and drain the device."""
    print(f"[{tag}] capture failed, staying eager: {e}")
    if os.environ.get("QA_DEBUG_GRAPH"):
        traceback.print_exception(type(e), e, e.__traceback__)
    torch.cuda.synchronize()


def record_data_parallel(front, apply, acc, params, world, pool):
    """A data-parallel optimiser step as TWO graphs around the gradient collective, which stays an ordinary launch:
    [`front()` -> (kl, stats): gather .. backward; gradients of `params` + KL packed into one flat bucket that lives in `pool`]
    -> all-reduce(bucket) -> [mean over `world` ranks, unpack onto the gradients, `apply(kl)`: clip, LR rule, Adam; `acc` += stats].
    `stats` is a tensor or a sequence of scalars (stacked inside the first graph).  Returns (ga, gb, bucket)."""
    def pack():
        kl, stats = front()
        grads = [p.grad for p in params if p.grad is not None]
        packed = grads + [kl.detach().reshape(1)]
        bucket = torch._utils._flatten_dense_tensors(packed)
        return grads, packed, bucket, stats if torch.is_tensor(stats) else torch.stack(list(stats))

    ga, (grads, packed, bucket, stats) = record(pack, pool=pool)

    def unpack():
        bucket.div_(world)
        parts = torch._utils._unflatten_dense_tensors(bucket, packed)
        torch._foreach_copy_(grads, list(parts[:len(grads)]))
        apply(parts[-1].reshape(()))
        acc.add_(stats)

    gb, _ = record(unpack, pool=pool)
    return ga, gb, bucket


def replay_step(ga, gb, bucket, grad_sync):
    """One recorded optimiser step: a single graph (`gb` None), or the pair of record_data_parallel around `grad_sync.all_reduce_`."""
    ga.replay()
    if gb is not None:
        grad_sync.all_reduce_(bucket)
        gb.replay()


def accumulate(acc, stats):
    """a step's logged values onto its accumulator: ONE tensor (add_), or a sequence of device scalars (one launch, fused.accumulate_scalars)"""
    if torch.is_tensor(stats):
        acc.add_(stats)
    else:
        from quadrupedal_agility_amd.rsl_rl.algorithms import fused
        fused.accumulate_scalars(acc, list(stats))


class MinibatchSchedule(list):
    """The recorded minibatch schedule of an update: `nmb` minibatches of `mb` rows by ONE permutation of the first nmb * mb rows of `srcs` (rows
    past that are never sampled), stepped through `epochs` times.  As a list it is the recorded steps, [(ga, gb, bucket)] as replay_step takes
    them -- what a learner keeps in its graph slot; everything a replay reads and no module owns hangs off it (feeding buffers, accumulator
    `acc`, data-parallel statistics and whatever the site puts into `held`) and so lives exactly as long as the slot's value.
    Feeding by permuted slots (`permuted`): persistent (nmb * mb, width) copies of the sources (1-D: width 1), filled in permuted order by one
    gather per update; minibatch i is `slot(i)`, rows [i mb, (i + 1) mb) of every copy.  By index buffer: a persistent (mb,) int64 tensor `idx`
    the recorded step gathers through; the host copies the next slice of the permutation into it before every replay."""

    def __init__(self, nmb, mb, srcs, permuted):
        super().__init__()
        self.nmb, self.mb, self.srcs, self.held, self.acc = nmb, mb, list(srcs), [], None
        dev = self.srcs[0].device
        self.idx = None if permuted else torch.zeros(mb, dtype=torch.int64, device=dev)
        self.bufs = [torch.empty(nmb * mb, x.shape[1] if x.dim() == 2 else 1, dtype=torch.float32, device=dev) for x in self.srcs] if permuted else None

    def slot(self, i):
        return [b[i * self.mb:(i + 1) * self.mb] for b in self.bufs]

    def feeds(self):
        """what `front` is called with, per recording: the views of each slot, or the index buffer"""
        return [self.slot(i) for i in range(self.nmb)] if self.bufs is not None else [(self.idx,)]

    def fill(self, perm):
        from quadrupedal_agility_amd.rsl_rl.algorithms import fused
        fused.gather_rows(perm, self.srcs, dsts=self.bufs)

    def record_steps(self, front, apply, acc, zero_grads=None, epoch=False, sync=None, params=None):
        """Record the step `front(*feed) -> (kl, stats)`, `apply(kl)`, `acc` += stats in one of three forms, all in one graph pool (the recordings
        never run concurrently): one recording per feed; `epoch`: the slots of an epoch as ONE recording, `zero_grads()` after each; `sync` (a
        GradSync): per feed the pair of record_data_parallel over `params`.  After the recording of a permuted slot `zero_grads()`: the next creates its own."""
        self.acc, pool = acc, torch.cuda.graph_pool_handle()

        def step(feed):
            kl, stats = front(*feed)
            apply(kl)
            accumulate(acc, stats)

        def all_slots():
            for feed in self.feeds():
                step(feed)
                zero_grads()

        def stacked(feed):          # the statistics as ONE tensor held here: every replay of the second graph reads it
            kl, stats = front(*feed)
            self.held.append(stats if torch.is_tensor(stats) else torch.stack(list(stats)))
            return kl, self.held[-1]

        if epoch:
            self.append((record(all_slots, pool=pool)[0], None, None))
            return
        for feed in self.feeds():
            if sync is None:
                self.append((record(lambda: step(feed), pool=pool)[0], None, None))
            else:
                self.append(record_data_parallel(lambda: stacked(feed), apply, acc, params, sync.world, pool))
            if self.bufs is not None:
                zero_grads()

    def run(self, perm, epochs, grad_sync=None):
        """One update: the permuted copies filled once and every recording replayed per epoch; or per minibatch the index slice copied, the one recording replayed"""
        if self.bufs is not None:
            self.fill(perm)
        for _ in range(epochs):
            if self.bufs is not None:
                for step in self:
                    replay_step(*step, grad_sync)
            else:
                for i in range(self.nmb):
                    self.idx.copy_(perm[i * self.mb:(i + 1) * self.mb])
                    replay_step(*self[0], grad_sync)
