"""Recording launches into hipGraphs: the ceremony every recorded path of both trees shares (rollouts, PPO / discriminator / DAgger steps,
the vision student's env step).  What a site records, what it synchronises, zeroes or warms up first, and what it does once a capture has
failed (mark its slot False, run the eager loop) stay at the site."""
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
