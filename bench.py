#!/usr/bin/env python3
"""bench.py -- env-steps/s of the Go2 BBC training loop on MI355X (BASELINE.json metric).

One "step" = one full PPO iteration of the hot path: 24 fused env steps for every env (HIP
kernel: 4 physics substeps + termination + 14 rewards + reset + 671-float observation), rollout
inference, fused GAE (HIP), 5 epochs x 4 minibatches of PPO + estimator updates.  Nothing is
skipped inside the timed region.  value = num_envs x 24 x steps x n_gpus / wall time.

  python bench.py --gpus 1 --steps 10 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times the steps, writes --dump-outputs if asked and prints the line: the
headline and what follows from the timed region alone.  --full also measures, after the timed region: the
rollout / update split, `roofline` and `policy_roofline` (the fused env-step and policy kernels, timed live
with events on the launch stream) and `cpu_baseline` (the CPU oracle's env step and whole torch-CPU
iterations on the host cores, bounded samples; not with --no_cpu_baseline).

  python bench.py --gpus 1 --steps 20 --warmup 5 --full
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ALG_BYTES_PER_ENV_STEP = 6166          # 2,648 B read + 3,518 B written per env-step (BBC)
HBM_PEAK_GBS = 8000.0                  # MI355X_MICROARCH.md: 8 TB/s HBM3E spec peak (6.3 TB/s achievable)
FP32_MFMA_PEAK_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense, exact f32
# Algorithmic learner FLOPs per sample (2 x MAC), DESIGN.md section 6: forward MACs actor 217,088, privileged encoder
# 3,712 (evaluated twice in the update), critic 507,520, estimator 15,744, history encoder 28,770 (forward only, no_grad)
_FWD = 217088 + 2 * 3712 + 507520 + 15744
UPDATE_FLOPS_PER_SAMPLE = 2 * (3 * _FWD - 343552 - 7296) + 2 * 28770      # fwd + dW + dx; no dx for the two first layers fed by raw observations
ROLLOUT_FLOPS_PER_SAMPLE = 2 * (217088 + 3712 + 507520 + 15744)


_RESULT_OUT = sys.stdout


def _self_launch(n):
    """`python bench.py --gpus N` without a launcher (how the driver calls it: BENCH_r05.json `cmd`): start the N ranks ourselves, one process
    per GPU under torch.distributed.run on 127.0.0.1, and pass their output through -- rank 0 prints the one JSON line.  Refuses, with the
    reason, when the box has fewer than N GPUs (unless QA_BENCH_SHARED_GPU=1: the N-ranks-on-one-GPU harness, gloo collectives)."""
    import socket
    import subprocess
    check = "--launch_check" in sys.argv
    if not check:
        import torch
        have = torch.cuda.device_count()
        if have < n and os.environ.get("QA_BENCH_SHARED_GPU") != "1":
            print(f"bench.py --gpus {n}: this box has {have} GPU(s).  One process per GPU needs {n}; QA_BENCH_SHARED_GPU=1 runs the {n} ranks on GPU 0 "
                  "over gloo (a harness for the data-parallel code path, not a scaling measurement).", file=sys.stderr)
            return 2
    with socket.socket() as sk:           # a free port for the rendezvous (the container's hostname may not resolve: 127.0.0.1 throughout)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def _launch_check(world, rank):
    """--launch_check: the ranks meet over gloo, agree on who is there, rank 0 prints one line.  No GPU, no library build."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.zeros(world, dtype=torch.int64)
    t[rank] = os.getpid()
    dist.all_reduce(t)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks": world, "pids": t.tolist(), "launcher": "bench.py self-launch" if os.environ.get("TORCHELASTIC_RUN_ID") else "external"}),
              file=_RESULT_OUT, flush=True)


def _collective_name(shared):
    """what carried the buckets: 'rccl <version>' or 'gloo'"""
    import torch
    if shared:
        return "gloo (host memory)"
    try:
        v = torch.cuda.nccl.version()
        return "rccl " + ".".join(str(x) for x in v)
    except Exception as e:      # never fatal for a bench line
        return f"rccl (version unavailable: {e})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num_envs", type=int, default=4096, help="envs of the whole job with --scaling strong (BASELINE metric: 4096), envs per GPU with --scaling weak")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong (default, the BASELINE metric and SURVEY 8e): --num_envs envs in total, rank r owns [r N/W, (r+1) N/W); "
                         "weak: --num_envs envs on every GPU")
    ap.add_argument("--amp", action="store_true", help="BASELINE config 3: discriminator + mocap reset on the real Go2 clips (baked dataset shipped with the package)")
    ap.add_argument("--terrain", default="plane", choices=["plane", "trimesh"],
                    help="plane = BASELINE configs 1-2 (flat terrain); trimesh = the reference's 10x40 tile course as a height field")
    ap.add_argument("--vision", action="store_true", help="with --tsc: the depth student (BASELINE configs[4]: --use_camera, 4096 envs in total)")
    ap.add_argument("--tsc", action="store_true", help="BASELINE config 4: TSC teacher on the agility course (two-level rollout, hybrid PPO); "
                    "--num_envs is per GPU (8192 over 8 GPUs = 1024 per GPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the rollout / update split, the env-side and policy kernels against their rooflines and, "
                         "on one GPU, the CPU baseline (a minute or more); a plain run reports the timed steps alone")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no_graph", action="store_true", help="launch the rollout eagerly instead of replaying a hipGraph")
    ap.add_argument("--cpu_seconds", type=float, default=12.0, help="with --full: the CPU baseline's budget for its rollout-only legs")
    ap.add_argument("--launch_check", action="store_true", help="plumbing check without a GPU: launch the ranks, rendezvous over gloo, print one line, exit")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (the networks' parameters and buffers, the rollout storage) "
                         "as DIR/<name>.npy, float32 / float64, at most 64 MB in all (larger arrays as a fixed seeded sample; DIR/manifest.json says which)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_self_launch(args.gpus))

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    global _RESULT_OUT
    _RESULT_OUT, sys.stdout = sys.stdout, sys.stderr       # stdout carries the ONE JSON line; the libraries' chatter goes to stderr
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE is {world}: one process per GPU (plain `python bench.py --gpus N` launches them itself)")
    if args.launch_check:
        return _launch_check(world, rank)
    # QA_BENCH_SHARED_GPU=1 (a harness, NOT a scaling measurement): every rank of the job runs on GPU 0 and the buckets travel over gloo.
    # What it bounds on a 1-GPU box: the cost of the data-parallel code path itself -- the PPO step as two graphs around a collective, the
    # per-rank shards, 20 collectives per iteration -- when no multi-GPU node is available.  The line says so (`shared_gpu_harness`).
    shared = os.environ.get("QA_BENCH_SHARED_GPU") == "1" and world > 1
    if shared:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    forced_dp = os.environ.get("QA_FORCE_DATA_PARALLEL") == "1" and "MASTER_ADDR" in os.environ     # dev: DP code path on one GPU
    if shared:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif world > 1 or forced_dp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device(dev), rank=rank, world_size=world)

    import __graft_entry__ as g
    if rank == 0:
        g.build()
    if world > 1:
        dist.barrier()
    if args.tsc:
        return bench_tsc(args, world, rank, local_rank, dev)
    from quadrupedal_agility_amd.legged_gym.envs import task_registry  # noqa: F401  (registers tasks)
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args

    if args.scaling == "strong" and args.num_envs % world:
        raise SystemExit(f"--num_envs {args.num_envs} does not split over {world} ranks")
    per_rank = args.num_envs // world if args.scaling == "strong" else args.num_envs
    total_envs = per_rank * world
    args.num_envs = per_rank                         # from here on: envs of THIS rank
    cfg = Go2LocomotionCfg()
    cfg.env.num_envs = per_rank
    cfg.env.env_id_offset, cfg.env.num_envs_global = rank * per_rank, total_envs      # random draws keyed by the global env id: the same job at any world size
    cfg.terrain.mesh_type = args.terrain
    cfg.env.mocap_state_init = bool(args.amp)
    cfg.seed = 1
    tcfg = Go2LocomotionCfgAlgo()
    tcfg.runner.amp_enabled = bool(args.amp)
    tcfg.runner.rollout_graph = not args.no_graph
    cli = get_args(["--device", "gpu", "--device_id", str(local_rank)])
    torch.manual_seed(1)
    env, _ = task_registry.make_env("go2_locomotion", args=cli, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=cli, train_cfg=tcfg, log_root=None)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # All recorded launches (rollout, PPO step, and their every-20th-iteration DAgger variants) are captured during the
    # first 21 iterations; they are run untimed here whatever W is, so that the timed region measures steady state
    # (a capture costs ~0.2 s once).  The W warm-up steps the contract asks for follow.
    pre = max(0, 21 - args.warmup)
    if pre:
        runner.learn(pre, init_at_random_ep_len=True)
    runner.learn(args.warmup, init_at_random_ep_len=(pre == 0))
    coll, lrn = [], []
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.learn(1, init_at_random_ep_len=False)
        coll.append(runner.last_perf["collection_time"]); lrn.append(runner.last_perf["learn_time"])
    if os.environ.get("QA_BENCH_TRACE") and rank == 0:
        print("per-iteration ms:", " ".join(f"{(c + l) * 1e3:.1f}" for c, l in zip(coll, lrn)), file=sys.stderr)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:                # before --full's kernel timings and rollouts, which overwrite the storage
        dump_outputs(args.dump_outputs, timed_outputs(runner))
    full = bbc_full(g, args, env, runner, dt, world, dev) if args.full else {}      # every rank: each times its own kernels
    T = runner.num_steps_per_env
    env_steps = args.num_envs * T * args.steps * world
    value = env_steps / dt

    if rank == 0:
        out = {
            "metric": "env-steps/sec (4096 Go2 envs) + wall-clock to 1k PPO iters, 1/2/4/8 GPU",
            "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": (f"go2_locomotion BBC + AMP (5 mocap gaits, {getattr(env, 'mocap_source', 'none')} clips: 17 labelled + 295 unlabelled), " if args.amp else
                                    "go2_locomotion BBC, discriminator off, default-pose reset, ") +
                                   f"{total_envs} envs in total = {args.num_envs} envs/GPU x {world}, {'plane' if args.terrain == 'plane' else 'height-field (trimesh course)'} terrain, 24 steps/iter, 5 epochs x 4 minibatches",
                       "num_envs_total": total_envs, "num_envs_per_gpu": args.num_envs, "steps_per_iter": T, "parallelism": f"dp{world}"},
            "wallclock_1k_iters_s": dt / args.steps * 1000.0,
            **({"ranks": world, "collective": _collective_name(shared)} if world > 1 else {}),
            **({"shared_gpu_harness": f"{world} ranks on ONE GPU, gloo collectives through host memory: bounds the data-parallel code path's own cost, says nothing about xGMI scaling",
                "n_gpus": 1, "ranks": world} if shared else {}),
            **full,
        }
        epochs, nmb = runner.alg.num_learning_epochs, runner.alg.num_mini_batches
        samples = args.num_envs * T
        if not args.amp:      # the discriminator's GEMMs are not counted, so the figure would overstate the AMP config
            lf = samples * (epochs * UPDATE_FLOPS_PER_SAMPLE + ROLLOUT_FLOPS_PER_SAMPLE)
            out["learner_roofline"] = {"bound": "mfma", "dtype": "f32", "achieved": lf / (dt / args.steps) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS,
                                       "unit": "TFLOP/s", "frac": lf / (dt / args.steps) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                       "algorithmic_flops_per_iteration": lf,
                                       "note": f"whole iteration time; {epochs} epochs x {nmb} minibatches of {samples // nmb} samples, GEMMs through hipBLASLt (fp32 MFMA 16x16x4)"}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.num_envs, args.cpu_seconds)
    if world > 1 or forced_dp:
        dist.destroy_process_group()
    if rank == 0:
        # RCCL's start-up banner sits in the C library's stdout buffer until somebody flushes it: do that first so the
        # JSON line is the LAST line of output
        import ctypes
        ctypes.CDLL(None).fflush(None)
        print(json.dumps(out), file=_RESULT_OUT, flush=True)


def bbc_full(g, args, env, runner, dt, world, dev):
    """--full, after the timed region of the behaviour-level bench: the rollout / update split and the env-step and policy kernels
    timed live against their rooflines.  The keys it adds to the JSON line."""
    import torch
    sim, T = env.sim, runner.num_steps_per_env
    # live timing of the fused env-step kernel: HIP events around single launches on the launch stream, same process,
    # same env state, right after the timed region (inside it the 24 steps of a rollout replay as ONE hipGraph launch,
    # which leaves no place for per-kernel events; profiles/ holds the rocprofv3 per-kernel average of the same command)
    act = torch.zeros(args.num_envs, 12, device=dev)
    sim.global_step = env.common_step_counter
    if hasattr(runner, "_lean_mask_for"):              # learn() restores the full exports when it returns (r5); time the kernel variant it launched
        env.set_lean_exports(runner._lean_mask_for(env))
    reps, per = 5, 40
    spans = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):                           # back-to-back launches of the kernel alone (no wrapper bookkeeping);
            sim.step(act, env.delay)                   # HIP events bracket the batch on the launch stream
        e1.record()
        spans.append((e0, e1))
    torch.cuda.synchronize()
    kern_ms_alone = sorted(a.elapsed_time(b) for a, b in spans)[reps // 2] / per
    # ... and as it runs inside a rollout: one event pair per launch, with the policy kernel (which sweeps 3 MB of weights and
    # the observation rows through L2) between two env steps.  This is the figure the rocprofv3 average of the whole
    # command corresponds to, and the one the roofline object uses.
    chain0 = runner._policy_chain()
    obs_now = env.get_observations()
    pairs = []
    for _ in range(reps * per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sim.step(act, env.delay)
        e1.record()
        pairs.append((e0, e1))
        if chain0 is not None and chain0.packed is not None:
            chain0.forward(obs_now)
    torch.cuda.synchronize()
    kern_ms = sorted(a.elapsed_time(b) for a, b in pairs)[len(pairs) // 2]
    # the two phases of an iteration, measured apart AFTER the timed region (inside it the host never waits for the GPU, so
    # per-phase host clocks mean nothing there): 5 rollouts alone, bracketed by synchronize; the update is the remainder
    roll = []
    for _ in range(5):
        torch.cuda.synchronize(); t1 = time.perf_counter()
        runner._collect(False, False)
        torch.cuda.synchronize(); roll.append(time.perf_counter() - t1)
        runner.alg.storage.clear()
    coll_s = sorted(roll)[len(roll) // 2]
    # live timing of the policy-inference kernel (qa_mlp_forward), same recipe as the env-step kernel
    chain, mlp_ms = runner._policy_chain(), None
    if chain is not None and chain.packed is not None:
        obs_now = env.get_observations()
        spans = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                chain.forward(obs_now)
            e1.record()
            spans.append((e0, e1))
        torch.cuda.synchronize()
        mlp_ms = sorted(a.elapsed_time(b) for a, b in spans)[reps // 2] / per
    achieved = ALG_BYTES_PER_ENV_STEP * args.num_envs / (kern_ms * 1e-3) / 1e9
    # the PMC pass on file is of the PLANE kernel with the lean export mask of a run without the discriminator (3); config 3 launches mask 1, the
    # trimesh course the height-field kernel: neither is the kernel that was counted
    if args.terrain != "plane" or args.amp:
        traffic, traffic_note = None, "the PMC pass on file is of the plane kernel with lean exports 3 (config 2); this run launches another variant of the kernel"
    else:
        traffic, traffic_note = _stamped_traffic(g, args.num_envs)
    out = {
        "rollout_env_steps_per_s": args.num_envs * T * world / coll_s,
        "collection_s": coll_s, "learn_s": dt / args.steps - coll_s,
        "roofline": {"kernel": "qa_env_step_kernel", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_note, "kernel_ms": kern_ms, "kernel_ms_back_to_back": kern_ms_alone, "rollout_graph": bool(getattr(runner, "_graph", None) is not None),
                     "algorithmic_bytes_per_launch": ALG_BYTES_PER_ENV_STEP * args.num_envs,
                     "note": "not byte-bound: 4096 envs = 256 workgroups = one per CU; the env's own wavefront is instruction-issue-bound (a Gauss-Seidel chain), r5 gives each workgroup two helper wavefronts on the CU's idle SIMDs for the substep's side chains, the non-foot rows, the history shift and the closing stores (69 -> 56 us back to back, DESIGN.md 4.1c, profiles/r5_env_step_helper_wavefronts.txt); traffic is the PMC figure of the lean-export kernel a training run launches (1.09x algorithmic); 16384 envs/GPU: 136 us per launch = 1.65x this rate (one-wavefront kernels: every SIMD has an env wavefront of its own there)"},
    }
    if mlp_ms is not None:
        pf = ROLLOUT_FLOPS_PER_SAMPLE * args.num_envs
        out["policy_roofline"] = {"kernel": "qa_mlp_forward_kernel", "bound": "mfma", "dtype": "f32", "achieved": pf / (mlp_ms * 1e-3) / 1e12,
                                  "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": pf / (mlp_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                  "kernel_ms": mlp_ms, "algorithmic_flops_per_launch": pf,
                                  "note": "estimator + privileged encoder + actor + critic of one env step in one launch, activations in LDS (DESIGN.md 4.11)"}
    return out


ENV_KERNEL_SOURCES = ("qa_sim.hip", "qa_physics.h", "qa_device.h", "qa_go2_model.h")


def env_kernel_hash(g):
    """hash of the sources the env-step kernel is compiled from (what a PMC traffic figure is valid for)"""
    return g._src_hash([os.path.join(g.CSRC, f) for f in ENV_KERNEL_SOURCES])[:16]


def _stamped_traffic(g, num_envs, name="env_step_traffic.json"):
    """roofline.traffic: the HBM bytes per launch of the PMC passes (tools/final_measure.sh -> profiles/env_step_traffic.json), reported only
    when that file was measured on the kernel sources this run built AND at this run's env count -- a figure from another version of the
    kernel, or from another launch size, is not a measurement of this one.  Counter passes cannot run inside
    this process: rocprofv3 collects them per process, in passes of their own."""
    prof = os.path.join(ROOT, "profiles", name)
    try:
        d = json.load(open(prof))
    except Exception:
        return None, "no PMC pass on file"
    if int(d.get("num_envs", -1)) != int(num_envs):
        return None, f"profiles/{name} was measured at {d.get('num_envs')} envs per launch, this run launches {num_envs}: no traffic figure for this size"
    if d.get("kernel_source_hash") != env_kernel_hash(g):
        return None, f"profiles/{name} was measured on kernel sources {d.get('kernel_source_hash', 'unstamped')}, this build is {env_kernel_hash(g)}: re-run tools/final_measure.sh"
    if d.get("fetch_correction") not in (1, 2):
        return None, f"profiles/{name} derives a fetch correction of {d.get('fetch_correction')} (the guide's factor is 2, an exact counter would give 1): its calibration was misread, the figure is void"
    return d.get("hbm_bytes_per_launch"), f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes on kernel sources {d['kernel_source_hash']} (tools/final_measure.sh)"


DUMP_BUDGET_BYTES = 60 << 20          # --dump-outputs: the arrays' data; the .npy headers and the manifest stay far below the rest of 64 MB


def timed_outputs(runner, storage=True):
    """what a caller of runner.learn() holds after the last timed iteration: the parameters and buffers of the networks it trains and the
    rollout storage that iteration filled (observations, actions, rewards, values, returns, advantages, ...; not with storage=False: the
    depth student's iteration does not fill it).  Name -> tensor."""
    import torch
    alg, out = runner.alg, {}
    for mod in ("actor_critic", "estimator", "disc", "depth_encoder", "depth_actor"):
        m = getattr(alg, mod, None)
        if isinstance(m, torch.nn.Module):
            out.update((f"{mod}.{k}", v) for k, v in m.state_dict().items() if torch.is_tensor(v))
    for k, v in (vars(alg.storage).items() if storage else ()):
        if torch.is_tensor(v) and not k.startswith("_") and v.dim() and not any(v is w for w in out.values()):      # privileged rows may alias the actor's
            out["storage." + k] = v
    return out


def dump_outputs(path, tensors):
    """writes every tensor as <path>/<name>.npy: float64 stays float64, integer tensors become float64, the rest float32.  Within
    DUMP_BUDGET_BYTES: the arrays in ascending size each get an equal share of what the smaller ones left; an array over its share is
    written as a sample of its elements -- flat indices drawn from a generator seeded by the name (so the same in every run of the same
    shapes), sorted, duplicates dropped.  <path>/manifest.json lists shape, dtype and, for samples, the seed and element count."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)

    def dtype(t):
        return np.float64 if t.dtype in (torch.float64, torch.int64, torch.int32) else np.float32

    items = sorted(tensors.items(), key=lambda kv: (kv[1].numel() * np.dtype(dtype(kv[1])).itemsize, kv[0]))
    left, manifest = DUMP_BUDGET_BYTES, {}
    for i, (name, t) in enumerate(items):
        dt = dtype(t)
        share = left // (len(items) - i)
        entry = {"shape": list(t.shape), "dtype": np.dtype(dt).name}
        t = t.detach()
        if t.numel() * np.dtype(dt).itemsize <= share:
            arr = t.cpu().numpy().astype(dt)
        else:
            seed = zlib.crc32(name.encode())
            draws = share // np.dtype(dt).itemsize
            flat = np.unique(np.random.default_rng(seed).integers(0, t.numel(), draws))
            idx = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(t.device) for a in np.unravel_index(flat, tuple(t.shape)))
            arr = t[idx].cpu().numpy().astype(dt)
            entry["sample"] = {"elements": int(arr.size), "of": int(t.numel()), "seed": seed, "draws": int(draws),
                               "index": "np.unique(np.random.default_rng(seed).integers(0, of, draws)), C-order flat indices"}
        np.save(os.path.join(path, name + ".npy"), arr)
        left -= arr.nbytes
        manifest[name] = entry
    with open(os.path.join(path, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


def _barrier_sync(world):
    import torch
    import torch.distributed as dist
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize()


def _max_over_ranks(dt, world, dev):
    import torch
    import torch.distributed as dist
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


DEPTH_ALG_BYTES_PER_ENV_STEP = 3 * 58 * 87 * 4   # the image ring: read slot 1, write slots 0 and 1 (the maps are read through L2)
TSC_ALG_BYTES_PER_ENV_STEP = 7300       # obs 800 x 4, 132 int16 scan lookups + 8 edge-mask lookups on top of the BBC figure


def bench_tsc(args, world, rank, local_rank, dev):
    """BASELINE configs 3 / 4 (indices of BASELINE.json `configs`): the task-level tree.
      --tsc           TSC teacher, 8192 envs in total: one step = one learn_RL iteration -- 24 x (task policy -> set_commands -> frozen
                      behaviour policy -> physics step on the obstacle course -> goal step -> reset -> observations -> discriminator
                      reward), GAE, 5 epochs x 4 minibatches of the hybrid PPO.
      --tsc --vision  TSC student with the depth camera, 4096 envs in total: one step = one learn_vision iteration -- 24 x (depth encoder
                      -> student actor -> set_commands -> behaviour policy -> physics -> goal step -> reset -> depth ray-cast ->
                      observations), one DAgger update + 6 BYOL minibatches.
    One process per GPU; with --scaling strong (default) the job's envs are split over the ranks, which exchange ONE flat gradient
    bucket per optimiser step (GradSync), the KL mean and the advantage moments; each rank builds ITS envs of the job's one course (the
    same obstacles at every world size)."""
    import torch
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import class_to_dict
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg, Go2AgilityCfgPPO
    from quadrupedal_agility_amd.tsc.rsl_rl.runners import OnPolicyRunner
    total = args.num_envs if args.num_envs != 4096 or args.vision else 8192
    if args.scaling == "strong":
        if total % world:
            raise SystemExit(f"--num_envs {total} is not divisible by {world} ranks")
        n = total // world
    else:
        n, total = total, total * world
    cfg = Go2AgilityCfg()
    cfg.env.num_envs, cfg.seed, cfg.course_seed = n, 1, 1          # one course for the job: rank r builds envs [r n, (r+1) n) of it
    cfg.env.env_id_offset, cfg.env.num_envs_global = rank * n, total
    d = cfg.domain_rand                                    # the reference's command line for this config: --randomize_base_mass ... --randomize_start
    d.randomize_base_mass = d.randomize_base_com = d.push_robots = True
    cfg.obstacle.randomize_start = True
    cfg.depth.use_camera = bool(args.vision)
    tcfg = class_to_dict(Go2AgilityCfgPPO())
    tcfg["depth_encoder"]["if_depth"] = bool(args.vision)
    torch.manual_seed(1)                                   # same initial weights everywhere (and broadcast from rank 0 anyway)
    env = lr.LeggedRobot(cfg, sim_device=dev)
    runner = OnPolicyRunner(env, tcfg, log_dir=None, device=dev)
    torch.manual_seed(1 + 104729 * rank)                   # the ranks' action noise / start draws differ
    # as in the behaviour-level bench: the teacher's every-20th-iteration DAgger variant of the rollout is recorded at its second use (iteration 20);
    # those one-off captures run untimed whatever W is, and the timed region measures steady state -- with its share of DAgger iterations
    # (r6: `--steps 20 --warmup 5` had the capture inside the timed region: 31.2 ms per iteration against 24.5 with 8 + 3)
    pre = 0 if args.vision else max(0, 21 - max(args.warmup, 2))
    if pre:
        runner.learn(pre, init_at_random_ep_len=True)
    runner.learn(max(args.warmup, 2), init_at_random_ep_len=(pre == 0))
    _barrier_sync(world)
    t0 = time.perf_counter()
    iter_ms = []
    for _ in range(args.steps):
        t1 = time.perf_counter()
        runner.learn(1)
        if os.environ.get("QA_BENCH_TRACE"):
            torch.cuda.synchronize(); iter_ms.append((time.perf_counter() - t1) * 1e3)
    if iter_ms and rank == 0:
        print("per-iteration ms:", " ".join(f"{v:.1f}" for v in iter_ms), file=sys.stderr)
    _barrier_sync(world)
    dt = _max_over_ranks(time.perf_counter() - t0, world, dev)
    if args.dump_outputs and rank == 0:                # before --full's rollouts, which overwrite the storage
        dump_outputs(args.dump_outputs, timed_outputs(runner, storage=not args.vision))
    T = tcfg["depth_encoder"]["num_steps_per_env"] if args.vision else runner.num_steps_per_env
    full = tsc_full(args, env, runner, n, T, dt, world, dev) if args.full else {}      # every rank: each times its own kernels
    what = ("TSC-student with depth-camera obs (58x87 ray-cast depth image per env step, depth encoder + GRU + student actor, DAgger + BYOL)" if args.vision else
            "TSC-teacher agility course")
    out = {"metric": "env-steps/sec (4096 Go2 envs) + wall-clock to 1k PPO iters, 1/2/4/8 GPU", "value": n * T * args.steps * world / dt, "unit": "env-steps/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
           "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"{what} (6 obstacles/env as height-field + ceiling collision terrain, randomize_base_mass/com, push_robots, randomize_start, "
                                  f"action noise U(0.8,1.2), frozen behaviour policy + discriminator at their initial weights), {total} envs in total = {n} envs/GPU x {world}, "
                                  f"{T} steps/iter" + ("" if args.vision else ", 5 epochs x 4 minibatches"),
                      "num_envs_total": total, "num_envs_per_gpu": n, "steps_per_iter": T, "parallelism": f"dp{world}"},
           **full}
    if world > 1:
        out["ranks"], out["collective"] = world, _collective_name(os.environ.get("QA_BENCH_SHARED_GPU") == "1")
    if args.vision:
        out["vision"] = dict(runner.last_vision)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_tsc(min(n, 1024), args.cpu_seconds, bool(args.vision))
    if rank == 0:
        print(json.dumps(out), file=_RESULT_OUT, flush=True)


def tsc_full(args, env, runner, n, T, dt, world, dev):
    """--full, after the timed region of the task-level bench: the rollout / update split, the env-side kernels of one step and the
    behaviour policy timed live against their rooflines.  The keys it adds to the JSON line."""
    import torch
    # the two phases of an iteration, measured apart AFTER the timed region between device syncs (inside it the host never waits for the
    # GPU -- a recorded rollout returns to the host in ~1 ms -- so the runner's own host clocks are not phase times)
    coll_s = None
    if not args.vision:
        roll = []
        for _ in range(5):
            torch.cuda.synchronize(); t1 = time.perf_counter()
            runner._collect(False, False)
            torch.cuda.synchronize(); roll.append(time.perf_counter() - t1)
            runner.alg.storage.clear()
        coll_s = sorted(roll)[len(roll) // 2]
    # the env-side kernels of one step, timed alone with HIP events on the launch stream
    act = torch.zeros(n, 12, device=dev)
    hist = torch.zeros(n, 8, 19, device=dev)
    spans = {}
    legs = [("physics", lambda: env.sim.physics_step(act, 1)),
            ("goal_step", lambda: env.bk.post_physics_step(env.root_states, env.contact_forces, env.rigid_body_states, hist, want_ids=False)),
            ("observations", lambda: env.bk.compute_observations(env.root_states, env.dof_pos, env.dof_vel, env.action_history_buf, env.rigid_body_states,
                                                                 env.mass_params_tensor, env.friction_coeffs_tensor, env.motor_strength))]
    if args.vision:
        legs.append(("depth", lambda: env.bk.update_depth_buffer(env.root_states, 1)))
    for name, fn in legs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(); e0.record()
        for _ in range(40):
            fn()
        e1.record(); torch.cuda.synchronize()
        spans[name] = e0.elapsed_time(e1) / 40
    kern_ms = sum(spans.values())
    alg_bytes = TSC_ALG_BYTES_PER_ENV_STEP + (DEPTH_ALG_BYTES_PER_ENV_STEP if args.vision else 0)
    achieved = alg_bytes * n / (kern_ms * 1e-3) / 1e9
    # r5: the task-level env step's HBM bytes from a stamped PMC pass of the same three kernels at THIS env count
    # (tools/final_measure.sh -> profiles/tsc_env_step_traffic.json), or null with the reason
    import __graft_entry__ as g
    sized = f"tsc_env_step_traffic_{n}.json"
    tsc_traffic, tsc_traffic_note = ((None, "no PMC pass of the depth kernel on file") if args.vision else
                                     _stamped_traffic(g, n, sized if os.path.exists(os.path.join(ROOT, "profiles", sized)) else "tsc_env_step_traffic.json"))
    if tsc_traffic is not None and tsc_traffic / (kern_ms * 1e-3) / 1e9 > HBM_PEAK_GBS:      # a figure that implies more than the HBM peak is not a measurement
        tsc_traffic, tsc_traffic_note = None, f"the figure on file ({tsc_traffic} B per env step) over {kern_ms * 1e3:.0f} us would be {tsc_traffic / (kern_ms * 1e-3) / 1e12:.1f} TB/s: void"
    out = {"collection_s": coll_s, "learn_s": (dt / args.steps - coll_s) if coll_s is not None else None,
           "rollout_env_steps_per_s": (n * T * world / coll_s) if coll_s is not None else None,
           "phase_split": "rollout alone between device syncs after the timed region (median of 5); update = iteration - rollout" if coll_s is not None else "not split (learn_vision interleaves env steps and the student's forward passes)",
           "roofline": {"kernel": "qa_env_step_kernel<false,4,1> + qa_tsc_goal_step + qa_tsc_observations" + (" + qa_tsc_depth_kernel" if args.vision else ""),
                        "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": tsc_traffic, "traffic_source": tsc_traffic_note, "kernel_ms": kern_ms, "kernel_ms_each": spans,
                        "algorithmic_bytes_per_launch": alg_bytes * n}}
    chain = getattr(runner, "_bbc_chain", None)
    if chain is not None and chain.packed is not None:      # the frozen behaviour policy of the two-level loop: one qa_mlp_forward launch per env step
        obs_bbc = env.get_observations_bbc()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        chain.forward(obs_bbc); e0.record()
        for _ in range(40):
            chain.forward(obs_bbc)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 40
        pf = 2 * (217088 + 28770) * n                     # actor 101-512-256-128-12 + history encoder (57->30 per frame, two temporal convolutions, 30->29), MACs x 2
        out["policy_roofline"] = {"kernel": "qa_mlp_forward_kernel (behaviour policy, history-encoder variant, no critic)", "bound": "mfma", "dtype": "f32",
                                  "achieved": pf / (ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                  "frac": pf / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, "kernel_ms": ms, "algorithmic_flops_per_launch": pf}
    return out


def cpu_baseline_tsc(num_envs, budget_s, vision):
    """the task-level env step on the host cores of this box: the oracle's physics on the agility course (OpenMP over envs) + the C twins of
    qa_tsc_goal_step / qa_tsc_reset / qa_tsc_observations (+ the depth ray-cast with --vision), driven through the same host code as the
    GPU env (tsc LeggedRobot on the oracle backend); bounded sample, no policy, no learner"""
    import torch
    from quadrupedal_agility_amd.tsc.legged_gym.envs.base import legged_robot as lr
    from quadrupedal_agility_amd.tsc.legged_gym.envs.go2.go2_agility_config import Go2AgilityCfg
    from quadrupedal_agility_amd.tsc.legged_gym.utils.obstacle import Obstacle
    from tests.oracle_backend import OracleBackend
    from tests.oracle_lib import load_oracle
    cores = _usable_cores()
    cfg = Go2AgilityCfg()
    cfg.env.num_envs, cfg.seed = num_envs, 1
    d = cfg.domain_rand
    d.randomize_base_mass = d.randomize_base_com = d.push_robots = True
    cfg.obstacle.randomize_start = True
    cfg.depth.use_camera = bool(vision)
    torch.manual_seed(1)
    ob = Obstacle(cfg.obstacle, num_envs, seed=1)
    env = lr.LeggedRobot(cfg, backend=OracleBackend(lr.make_qa_config(cfg, ob, seed=1)), bookkeeping_lib=(load_oracle(), "qo_"))
    act, hist = torch.zeros(num_envs, 12), torch.zeros(num_envs, 8, 19)
    env.step(act, hist)
    t0 = time.perf_counter(); k = 0
    while time.perf_counter() - t0 < budget_s:
        env.step(act, hist); k += 1
    dt = time.perf_counter() - t0
    return {"value": num_envs * k / dt, "unit": "env-steps/s", "cores": cores, "kind": "port",
            "sample": f"{k} task-level env steps of {num_envs} envs (oracle physics on the course + goal step + reset + observations" +
                      (" + depth ray-cast" if vision else "") + f", zero actions, no policy, no learner), OpenMP over envs, {dt:.1f} s"}


def cpu_baseline(num_envs, budget_s):
    """SURVEY 8d's host-CPU baseline on THIS box, same config / seed: (i) the CPU oracle's fused env step (same physics + env math,
    OpenMP over envs) alone, all cores and one core; (ii) whole PPO iterations of the same trainer with CPU physics (oracle) + torch-CPU
    learner (`torch.set_num_threads(nproc)`): 1 warm-up + 3 timed iterations -- rollout, learner and whole-iteration figures."""
    import numpy as np
    import torch
    from tests.oracle_lib import OracleSim, go2_cfg
    cores = _usable_cores()
    q = go2_cfg(num_envs, seed=1)
    o = OracleSim(q)
    o.reset_all()
    act = np.random.default_rng(0).normal(0, 0.3, (num_envs, 12)).astype(np.float32)
    o.step(act)
    t0 = time.perf_counter(); n = 0
    while time.perf_counter() - t0 < budget_s / 2:
        o.step(act); n += 1
    dt = time.perf_counter() - t0
    out = {"value": num_envs * n / dt, "unit": "env-steps/s", "cores": cores, "kind": "port",
           "sample": f"rollout only: {n} fused env steps of {num_envs} envs on plane terrain (physics + obs/reward, no policy, no learner), OpenMP over envs, {dt:.1f} s"}
    # the single-core figure SURVEY 8d asks for: the same steps with the OpenMP team held to one thread (~3 s)
    try:
        import ctypes
        gomp = ctypes.CDLL("libgomp.so.1")
        gomp.omp_set_num_threads(1)
        t0 = time.perf_counter(); n1 = 0
        while time.perf_counter() - t0 < 3.0:
            o.step(act); n1 += 1
        out["single_core_value"] = num_envs * n1 / (time.perf_counter() - t0)
        gomp.omp_set_num_threads(cores)
    except OSError:
        pass
    del o
    # ---- whole iterations on the CPU: oracle physics + torch-CPU policy / GAE / PPO (BASELINE config 2's settings).  In child
    # processes with their own thread budget and hard time limits: the baseline is a report, it must never cost the bench line and it
    # must never come back as an error record: a 512-env probe (1 warm-up + 1 iteration, seconds) runs first; the
    # full-size leg runs only if the probe says it fits its limit, and otherwise the probe's own rate is reported, labelled as such.
    threads = min(cores, 64)
    probe = _cpu_iteration_leg(512, 1, threads, 90)
    full = None
    if "iteration_s" in probe:
        est = probe["iteration_s"] * (num_envs / 512.0) * 3 + probe.get("startup_s", 10.0)      # 1 warm-up + 2 timed iterations
        if num_envs <= 512:
            full = probe
        elif est <= 100.0:
            full = _cpu_iteration_leg(num_envs, 2, threads, 150)
    if full is not None and "iteration_s" in full:
        out["iteration"] = full
    elif "iteration_s" in probe:
        out["iteration"] = dict(probe, extrapolated=True, iteration_s=probe["iteration_s"] * num_envs / 512.0,
                                rollout_s=probe["rollout_s"] * num_envs / 512.0, learner_s=probe["learner_s"] * num_envs / 512.0,
                                note=f"EXTRAPOLATED from a 512-env iteration on this box (env-steps/s taken as size-independent, times scaled by {num_envs}/512): "
                                     f"the {num_envs}-env leg would not fit its 150 s limit on {threads} threads here" +
                                     ("" if full is None else f" (it was tried: {full.get('why', 'no result')})"))
    else:
        out["iteration"] = {"value": None, "unit": "env-steps/s", "note": "the torch-CPU iteration leg produced no figure on this box, not even at 512 envs: " + probe.get("why", "?")}
    return out


def _usable_cores():
    """cores this process may run on (affinity mask / cpuset), not the machine's count"""
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        return os.cpu_count() or 1


def _cpu_iteration_leg(num_envs, its, threads, limit_s):
    import subprocess
    env_vars = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), QA_CPU_ITER_ENVS=str(num_envs), QA_CPU_ITER_ITS=str(its))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu_iteration_child"], env=env_vars, capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        return {"why": f"1 warm-up + {its} iterations of {num_envs} envs did not finish within {limit_s} s on {threads} threads"}
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not line:
        return {"why": (r.stderr or "no output")[-300:]}
    try:
        d = json.loads(line[-1])
    except ValueError:
        return {"why": "unparsable child output: " + line[-1][-200:]}
    if not isinstance(d, dict) or not isinstance(d.get("iteration_s"), (int, float)):      # e.g. an error record: never a KeyError in the baseline report
        return {"why": "the child printed no iteration_s: " + line[-1][-200:]}
    d["startup_s"] = max(0.0, (time.perf_counter() - t0) - d["iteration_s"] * (its + 1))
    return d


def cpu_iteration_child():
    """1 warm-up + 2 timed PPO iterations of BASELINE config 2 on the host: oracle physics (OpenMP) + torch-CPU learner"""
    import torch
    num_envs = int(os.environ.get("QA_CPU_ITER_ENVS", "4096"))
    its = int(os.environ.get("QA_CPU_ITER_ITS", "2"))
    threads = int(os.environ.get("OMP_NUM_THREADS", "8"))
    torch.set_num_threads(threads)
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import make_qa_config
    from tests.oracle_backend import OracleBackend
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = num_envs; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
    tcfg = Go2LocomotionCfgAlgo(); tcfg.runner.amp_enabled = False
    cli = get_args(["--device", "cpu"])
    torch.manual_seed(1)
    env, _ = task_registry.make_env("go2_locomotion", args=cli, env_cfg=cfg, backend=OracleBackend(make_qa_config(cfg, seed=1)))
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=cli, train_cfg=tcfg, log_root=None)
    runner.learn(1, init_at_random_ep_len=True)
    coll, lrn = [], []
    t0 = time.perf_counter()
    for _ in range(its):
        runner.learn(1)
        coll.append(runner.last_perf["collection_time"]); lrn.append(runner.last_perf["learn_time"])
    dt_it = (time.perf_counter() - t0) / its
    T = runner.num_steps_per_env
    print(json.dumps({"value": num_envs * T / dt_it, "unit": "env-steps/s", "iteration_s": dt_it, "rollout_s": sum(coll) / its, "learner_s": sum(lrn) / its,
                      "threads": threads,
                      "why_these_threads": "this leg is capped at min(cores, 64) threads (one NUMA-sized group for torch's intra-op pool; chosen in r2 to bound the "
                                           "leg inside its 150 s limit, not a measured optimum) while the rollout-only figure above uses every core: the oracle's env "
                                           "step is embarrassingly parallel over envs, the torch-CPU learner (90 % of this leg) is not",
                      "sample": f"{its} whole PPO iterations after 1 warm-up: {num_envs} envs x {T} steps of oracle physics + torch-CPU policy, GAE, 5 epochs x 4 minibatches, {threads} threads"}))


if __name__ == "__main__":
    if "--cpu_iteration_child" in sys.argv:
        cpu_iteration_child()
    else:
        main()
