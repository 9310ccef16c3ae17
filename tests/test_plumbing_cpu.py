"""BASELINE config 1: go2_locomotion BBC, 64 envs, plane, PPO on CPU physics (the oracle) + CPU torch.
Exercises the whole host-side mirror -- task registry, LeggedRobot views, runner, SSInfoGAIL update,
checkpoint round trip -- without a GPU."""
import os

import numpy as np
import pytest
import torch

from quadrupedal_agility_amd.legged_gym.envs import *  # noqa: F401,F403
from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
from quadrupedal_agility_amd.legged_gym.utils import get_args, task_registry
from quadrupedal_agility_amd.legged_gym.utils.cfg_to_c import make_qa_config
from tests.oracle_backend import OracleBackend


def make_env(n=64, mocap=False, amp=False):
    cfg = Go2LocomotionCfg()
    cfg.env.num_envs = n
    cfg.terrain.mesh_type = "plane"
    cfg.env.mocap_state_init = mocap
    cfg.seed = 1
    qc = make_qa_config(cfg, seed=1)
    if mocap:
        qc.num_mocap_frames = 5 * 4096
    args = get_args(["--device", "cpu", "--num_envs", str(n)])
    env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg, backend=OracleBackend(qc))
    return env, args


def test_env_api_surface():
    env, _ = make_env(16)
    assert (env.num_envs, env.num_obs, env.num_privileged_obs, env.num_obs_disc, env.num_actions) == (16, 101, 101, 49, 12)
    assert env.dt == pytest.approx(0.02) and env.max_episode_length == 1000 and env.dim_c == 5
    assert env.default_dof_pos.shape == (1, 12) and env.dof_pos_limits.shape == (12, 2)
    assert list(env.reward_scales.keys()) == sorted(env.reward_scales.keys()) and len(env.reward_names) == 14
    obs, priv = env.reset()
    assert obs.shape == (16, 671) and priv.shape == (16, 671) and env.get_disc_observations().shape == (16, 49)
    out = env.step(torch.zeros(16, 12))
    assert len(out) == 7 and out[2].shape == (16,) and out[3].dtype == torch.int64
    assert out[5].dtype == torch.int64 and out[6].shape[1] == 49
    # learner-written attributes go through to the engine
    env.prior_parameters = torch.tensor([0.5, 0.1, 0.1, 0.2, 0.1])
    assert np.allclose(env.sim.o.t["PRIOR_PARAMETERS"], [0.5, 0.1, 0.1, 0.2, 0.1])
    env.episode_length_buf = torch.full((16,), 7, dtype=torch.int64)
    assert (env.sim.o.t["EPISODE_LENGTH"] == 7).all()
    # views alias the arena: dof_pos is dof_state[..., 0]
    env.dof_pos[0, 0] = 0.123
    assert env.dof_state.view(16, 12, 2)[0, 0, 0] == pytest.approx(0.123)


def _train_cfg(amp):
    t = Go2LocomotionCfgAlgo()
    t.runner.amp_enabled = amp
    t.runner.num_preload_transitions = 2000
    t.algorithm.disc_replay_buffer_size = 20000
    t.runner.save_interval = 2
    return t


@pytest.mark.parametrize("amp", [False, True])
def test_learn_two_iterations_and_checkpoint(tmp_path, amp):
    torch.manual_seed(0)
    env, args = make_env(64, mocap=amp, amp=amp)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=_train_cfg(amp), log_root=str(tmp_path))
    before = {k: v.clone() for k, v in runner.alg.actor_critic.state_dict().items()}
    runner.learn(2, init_at_random_ep_len=True)
    after = runner.alg.actor_critic.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    assert all(torch.isfinite(v).all() for v in after.values())
    path = os.path.join(runner.log_dir, "model.pt")
    assert os.path.exists(path)
    ck = torch.load(path, weights_only=False)
    assert set(ck.keys()) == {"actor_critic", "estimator", "disc", "optim_ac", "optim_hist_encoder", "optim_estimator",
                              "optim_d", "optim_q_eps", "optim_q_c", "disc_normalizer", "reward_i_normalizer", "iter", "infos"}
    assert type(ck["disc_normalizer"]).__name__ == "Normalizer" and ck["disc_normalizer"].mean.shape == (98,)
    shapes = {k: tuple(v.shape) for k, v in ck["actor_critic"].items()}
    assert shapes["actor_trunk.0.weight"] == (512, 101) and shapes["critic_trunk.0.weight"] == (512, 671)
    assert shapes["history_encoder.conv_layers.0.weight"] == (20, 30, 4) and shapes["std"] == (12,)
    assert sum(v.numel() for v in ck["actor_critic"].values()) == 735699
    # round trip
    runner2, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=_train_cfg(amp), log_root=None)
    runner2.load(path)
    for k, v in runner2.alg.actor_critic.state_dict().items():
        assert torch.equal(v, after[k])
    assert os.path.exists(os.path.join(runner.log_dir, "scalars.jsonl")) or any(f.startswith("events") for f in os.listdir(runner.log_dir))


def test_replay_ring_insert_handles_wraps_and_oversized_batches():
    """ReplayBuffer.insert with whole rollouts (T*N rows per call, as the recorded rollout path does): against a plain list model of
    the ring -- partial fill, a single wrap, an exact fit, a batch larger than the ring (only its newest rows survive)"""
    import torch
    from quadrupedal_agility_amd.rsl_rl.storage import ReplayBuffer
    size = 50
    rb = ReplayBuffer(3, 5, 2, size, "cpu")          # obs_dim 3, dim_c 5, history 2 -> 6-wide rows
    model, pos, count, nxt = [None] * size, 0, 0, 0
    for n in (20, 20, 25, 50, 7, 120, 49, 1, 200):
        ids = torch.arange(nxt, nxt + n, dtype=torch.float32); nxt += n
        states = ids.view(n, 1).expand(n, 6).contiguous()
        rb.insert(states, ids.view(n, 1).clone(), ids.view(n, 1).expand(n, 5).contiguous())
        if n >= size:
            model, pos, count = list(ids[n - size:].tolist()), 0, size
        else:
            for v in ids.tolist():
                model[pos] = v; pos = (pos + 1) % size
            count = min(size, count + n)
        assert rb.num_samples == count and rb.step == pos
        got = rb.states[:, 0].tolist()
        assert all(m is None or g == m for g, m in zip(got, model))
        assert torch.equal(rb.latent_eps[:count, 0], rb.states[:count, 0]) and torch.equal(rb.latent_c[:count, 4], rb.states[:count, 5])


def test_buffers_that_recorded_launches_read_keep_their_addresses():
    """hipGraph replays read these tensors by address: the eager GAE fallback and the normaliser update must write them in place"""
    import torch
    from quadrupedal_agility_amd.rsl_rl.storage import RolloutStorage
    from quadrupedal_agility_amd.rsl_rl.utils.utils import TorchNormalizer
    st = RolloutStorage(8, 5, [11], [11], [3], "cpu")
    st.rewards.normal_(); st.values.normal_(); st.dones.zero_()
    before = (st.advantages.data_ptr(), st.returns.data_ptr())
    for _ in range(2):
        st.compute_returns(torch.randn(8, 1), 0.99, 0.95)
    assert (st.advantages.data_ptr(), st.returns.data_ptr()) == before
    assert abs(float(st.advantages.mean())) < 1e-5 and float(st.advantages.std()) == __import__("pytest").approx(1.0, abs=1e-4)
    nz = TorchNormalizer(4, "cpu")
    ptrs = (nz.mean.data_ptr(), nz.var.data_ptr(), nz.count.data_ptr())
    nz.update_torch([torch.randn(50, 4) * 3 + 1, torch.randn(20, 4)])
    assert (nz.mean.data_ptr(), nz.var.data_ptr(), nz.count.data_ptr()) == ptrs
    assert float(nz.count) == __import__("pytest").approx(70.0001, abs=1e-3) and float(nz.mean.abs().max()) > 0.1


# ------------------------------------------------------------------ rsl_rl/recording.py: the ceremony of recording a hipGraph, with the device faked
class _FakeCapture:
    """torch.cuda.CUDAGraph / torch.cuda.graph / torch.cuda.synchronize stand-ins: a `with` body runs at once on the CPU and `log` keeps what happened"""

    def __init__(self, monkeypatch):
        import contextlib
        import gc
        self.log = log = []

        class Graph:
            def replay(self):
                log.append(("replay", self))

        @contextlib.contextmanager
        def graph(g, pool=None, stream=None):
            log.append(("capture", g, pool, stream, gc.isenabled()))
            yield
            log.append(("end", g))

        monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
        monkeypatch.setattr(torch.cuda, "graph", graph)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append(("synchronize",)))


def test_no_gc_restores_the_collector():
    import gc
    from quadrupedal_agility_amd.rsl_rl import recording
    assert gc.isenabled()
    collections = []
    real = gc.collect
    try:
        gc.collect = lambda *a: collections.append(gc.isenabled()) or real(*a)
        with pytest.raises(KeyError):
            with recording.no_gc():
                assert not gc.isenabled()
                raise KeyError("body")
        assert gc.isenabled()                   # restored although the body raised
        assert collections == [True]            # one collection on entry, before the collector is switched off
        gc.disable()
        with recording.no_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()               # was off on entry: stays off
    finally:
        gc.collect = real
        gc.enable()


def test_record_runs_the_body_under_capture_and_returns_graph_and_result(monkeypatch):
    from quadrupedal_agility_amd.rsl_rl import recording
    fake = _FakeCapture(monkeypatch)
    g, out = recording.record(lambda: fake.log.append(("body",)) or 42, pool="POOL", stream="STREAM")
    assert isinstance(g, torch.cuda.CUDAGraph) and out == 42
    assert fake.log == [("capture", g, "POOL", "STREAM", False), ("body",), ("end", g)]      # collector off inside, nothing synchronised or zeroed for the caller
    fake.log.clear()
    g2, _ = recording.record(lambda: None)
    assert fake.log[0] == ("capture", g2, None, None, False) and g2 is not g
    with pytest.raises(ZeroDivisionError):      # a failing body is the site's to catch
        recording.record(lambda: 1 / 0)
    import gc
    assert gc.isenabled()


def test_capture_failed_prints_the_tagged_line_and_the_traceback_only_when_asked(monkeypatch, capsys):
    from quadrupedal_agility_amd.rsl_rl import recording
    fake = _FakeCapture(monkeypatch)

    def fail(tag):
        try:
            recording.record(lambda: {}["missing tensor"])
        except Exception as e:
            recording.capture_failed(tag, e)

    monkeypatch.delenv("QA_DEBUG_GRAPH", raising=False)
    fail("ppo update graph")
    out, err = capsys.readouterr()
    assert out == "[ppo update graph] capture failed, staying eager: 'missing tensor'\n"
    assert "Traceback" not in out + err
    assert fake.log[-1] == ("synchronize",) and fake.log.count(("synchronize",)) == 1
    monkeypatch.setenv("QA_DEBUG_GRAPH", "1")
    fail("tsc rollout graph")
    out, err = capsys.readouterr()
    assert out.startswith("[tsc rollout graph] capture failed, staying eager: 'missing tensor'\n")
    assert "Traceback (most recent call last)" in out + err and "KeyError: 'missing tensor'" in out + err and "in record" in out + err
    assert fake.log[-1] == ("synchronize",) and fake.log.count(("synchronize",)) == 2


def test_data_parallel_pair_packs_reduces_and_applies_in_order(monkeypatch):
    from quadrupedal_agility_amd.rsl_rl import recording
    fake = _FakeCapture(monkeypatch)
    log = fake.log
    for mod, name in ((torch._utils, "_flatten_dense_tensors"), (torch._utils, "_unflatten_dense_tensors"), (torch, "_foreach_copy_")):
        def wrapped(*a, _f=getattr(mod, name), _n=name):
            log.append((_n, a[0].clone() if torch.is_tensor(a[0]) else [t.clone() for t in a[0]]))
            return _f(*a)
        monkeypatch.setattr(mod, name, wrapped)
    params = [torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(5))]      # the last one gets no gradient
    g0, g1 = torch.arange(6.0).view(2, 3) + 1, torch.arange(4.0) - 8
    acc = torch.tensor([10.0, 20.0])

    def front():
        log.append(("front",))
        params[0].grad, params[1].grad = g0.clone(), g1.clone()
        return torch.tensor([[0.5]]), (torch.tensor(3.0), torch.tensor(4.0))

    def apply(kl):
        log.append(("apply", kl.clone(), params[0].grad.clone(), params[1].grad.clone(), acc.clone()))

    ga, gb, bucket = recording.record_data_parallel(front, apply, acc, params, 2, "POOL")
    names = [e[0] for e in log]
    assert names == ["capture", "front", "_flatten_dense_tensors", "end", "capture", "_unflatten_dense_tensors", "_foreach_copy_", "apply", "end"]
    assert log[0][1:4] == (ga, "POOL", None) and log[4][1:4] == (gb, "POOL", None) and ga is not gb
    flat = torch.cat([g0.view(-1), g1, torch.tensor([0.5])])
    assert bucket.shape == (11,) and torch.equal(bucket, flat / 2) and float(bucket[-1]) * 2 == 0.5       # [gradients | KL], the mean over the 2 ranks
    assert torch.equal(log[5][1], flat / 2)                                 # divided BEFORE it is unpacked
    assert torch.equal(log[6][1][0], g0) and torch.equal(log[6][1][1], g1)      # the copy's destinations are the parameters' own gradients ...
    _, kl, grad0, grad1, acc_then = log[7]
    assert kl.shape == () and float(kl) == 0.25
    assert torch.equal(grad0, g0 / 2) and torch.equal(grad1, g1 / 2)        # ... and they hold the mean when the optimiser runs
    assert torch.equal(acc_then, torch.tensor([10.0, 20.0])) and torch.equal(acc, torch.tensor([13.0, 24.0]))       # statistics (stacked) go on last
    assert params[0].grad.data_ptr() != bucket.data_ptr()

    class Sync:
        def all_reduce_(self, t):
            log.append(("all_reduce", t))

    log.clear()
    recording.replay_step(ga, gb, bucket, Sync())
    assert log == [("replay", ga), ("all_reduce", bucket), ("replay", gb)] and log[1][1] is bucket
    log.clear()
    recording.replay_step(ga, None, None, None)          # a step recorded as one graph
    assert log == [("replay", ga)]


# ------------------------------------------------------------------ the C-ABI call helper (_capi.Api)
class _StandIn:
    """what `_capi.Api` is handed in place of a library: entry points under a prefix, statuses as return values"""

    def __init__(self, with_error_text):
        self.seen = []
        if with_error_text:
            self.x_last_error = lambda: b"x_fail: the reason"

    def x_ok(self, *args):
        self.seen.append(args)
        return 0

    def x_fail(self, *args):
        self.seen.append(args)
        return -3


def test_call_helper_returns_normally_on_a_zero_status():
    from quadrupedal_agility_amd import _capi
    lib = _StandIn(True)
    api = _capi.Api(lib, "x_")
    assert api.launch("ok", 1, 2.5, on=torch.device("cpu")) is None and api.call("ok", 7) is None
    api.check("ok", 0)
    assert lib.seen == [(1, 2.5, None), (7,)]


@pytest.mark.parametrize("with_error_text", [True, False])
def test_call_helper_raises_with_name_code_and_error_text(with_error_text):
    from quadrupedal_agility_amd import _capi
    api = _capi.Api(_StandIn(with_error_text), "x_")
    text = "x_fail: the reason" if with_error_text else _capi.NO_ERROR_TEXT
    for run in (lambda: api.launch("fail", 1, on=torch.zeros(2)), lambda: api.call("fail", 1), lambda: api.check("fail", -3)):
        with pytest.raises(RuntimeError) as e:
            run()
        assert str(e.value) == f"x_fail failed with code -3: {text}"
    assert _capi.NO_ERROR_TEXT == "(an injected library: no error text)"


def test_call_helper_passes_no_stream_on_the_cpu_and_none_without_one():
    from quadrupedal_agility_amd import _capi
    lib = _StandIn(True)
    api = _capi.Api(lib, "x_")
    assert api.stream(torch.device("cpu")) is None and api.stream(torch.zeros(3)) is None
    api.launch("ok", "a", on=torch.device("cpu"))
    api.launch("ok", "b", on=torch.zeros(3))
    api.call("ok", "c", 4)
    assert lib.seen == [("a", None), ("b", None), ("c", 4)]          # the stream goes last; the no-stream variant appends nothing

