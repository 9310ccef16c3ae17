"""-m gpu: config 2 with a non-ELU policy end to end -- rollouts replayed from a hipGraph, PPO and DAgger steps recorded, no recording site falling
back -- and the recorded steps against the same steps launched eagerly (the mechanism of tests/test_gpu_train.py: same seed, the recorded paths
switched off by their `_*_graph = False` hooks).  The history encoder's gradients under hipGraph replay are compared with float64 autograd as well: a
stale bias sum (profiles/r2_hipgraph_stale_reductions.md) would be equal in the eager and the recorded run of one data set."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _runner(name, n=256):
    from quadrupedal_agility_amd.legged_gym.envs import task_registry
    from quadrupedal_agility_amd.legged_gym.envs.go2.go2_locomotion_config import Go2LocomotionCfg, Go2LocomotionCfgAlgo
    from quadrupedal_agility_amd.legged_gym.utils import get_args
    cfg = Go2LocomotionCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"; cfg.env.mocap_state_init = False; cfg.seed = 1
    t = Go2LocomotionCfgAlgo(); t.runner.amp_enabled = False
    t.policy.activation = name; t.estimator.activation = name
    args = get_args(["--device", "gpu"])
    torch.manual_seed(0)
    env, _ = task_registry.make_env("go2_locomotion", args=args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name="go2_locomotion", args=args, train_cfg=t, log_root=None)
    return env, runner


@pytest.mark.parametrize("name", ["tanh", "lrelu"])
def test_recorded_flow_equals_eager_flow(monkeypatch, name):
    from quadrupedal_agility_amd.rsl_rl import recording
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    failed = []
    monkeypatch.setattr(recording, "capture_failed", lambda tag, e: failed.append((tag, repr(e))))
    res = []
    for recorded in (True, False):
        env, runner = _runner(name)
        a = runner.alg
        assert fused.uniform_activation(a.actor_critic, a.estimator) is not None and a.use_update_graph
        if not recorded:
            a._ac_graph = False; a._dagger_graph = False
        runner.learn(3, init_at_random_ep_len=True)          # iteration 0 acts through the history encoder and runs the DAgger regression
        torch.cuda.synchronize()
        assert not failed, failed
        assert runner._graph is not None and not runner._graph_failed          # the rollouts were replays of a recorded launch sequence
        assert runner._policy_chain(False) is not None and runner._policy_chain(True) is not None
        assert a._train_chain_rows(256 * 24 // a.num_mini_batches) is not None
        assert (a._ac_graph not in (None, False)) == recorded
        res.append([p.detach().clone() for p in list(a.actor_critic.parameters()) + list(a.estimator.parameters())])
    assert all(torch.isfinite(x).all() for x in res[0])
    assert all(torch.equal(x, y) for x, y in zip(*res))


@pytest.mark.parametrize("name", ["tanh", "lrelu"])
def test_recorded_dagger_sessions_equal_eager_sessions(monkeypatch, name):
    """tests/test_gpu_train.py::test_recorded_dagger_sessions_equal_eager_sessions_on_new_data for a non-ELU history encoder"""
    from quadrupedal_agility_amd.rsl_rl import recording
    failed = []
    monkeypatch.setattr(recording, "capture_failed", lambda tag, e: failed.append((tag, repr(e))))
    env, runner = _runner(name)
    runner.learn(21, init_at_random_ep_len=True)             # DAgger at 0 (eager) and 20 (recorded + replayed)
    a = runner.alg
    assert not failed, failed
    assert a._dagger_graph not in (None, False) and set(runner._graphs) == {False, True} and not runner._graph_failed
    hp = list(a.actor_critic.history_encoder.parameters())
    st = a.optim_hist_encoder.state

    def snap():
        return [p.detach().clone() for p in hp], [{k: v.clone() for k, v in st[p].items()} for p in hp]

    def restore(s):
        with torch.no_grad():
            for p, q in zip(hp, s[0]): p.copy_(q)
            for p, d in zip(hp, s[1]):
                for k, v in d.items(): st[p][k].copy_(v)

    graph = a._dagger_graph
    for session in range(3):
        a.storage.observations.copy_(torch.randn_like(a.storage.observations) * (0.5 + session))
        start, rng = snap(), torch.cuda.get_rng_state()
        a.storage.step = a.storage.num_transitions_per_env
        loss_g = a.update_dagger(); got = [p.detach().clone() for p in hp]
        restore(start); torch.cuda.set_rng_state(rng)
        a.storage.step = a.storage.num_transitions_per_env
        a._dagger_graph = False
        loss_e = a.update_dagger(); want = [p.detach().clone() for p in hp]
        a._dagger_graph = graph
        assert loss_g == pytest.approx(loss_e, rel=1e-5)
        for (n, _), x, y in zip(a.actor_critic.history_encoder.named_parameters(), got, want):
            assert torch.allclose(x, y, rtol=1e-5, atol=1e-7), (session, n, float((x - y).abs().max()))
        assert any(not torch.equal(x, y) for x, y in zip(got, start[0]))


@pytest.mark.parametrize("name", ["tanh", "lrelu"])
def test_history_encoder_gradients_under_replay_equal_float64_autograd(name):
    """forward + backward of the history encoder recorded once and replayed on NEW data: every gradient, the biases' column sums included, equals
    float64 autograd on the data of that replay (bound: 3e-4 x max|grad|, or 3 x the error of torch's own fp32 modules)"""
    from quadrupedal_agility_amd.rsl_rl.modules import ActorCritic
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    torch.manual_seed(4)
    ac = ActorCritic(101, 671, 12, 57, 10, 4, 29, 11, actor_hidden_dims=[64], critic_hidden_dims=[64], priv_encoder_dims=[64], activation=name,
                     train_with_estimated_latent=True)
    he = ac.history_encoder
    he64, he32 = copy.deepcopy(he).double(), copy.deepcopy(he)
    he = he.cuda()
    params = list(he.parameters())
    rows = 6144
    x, gy = torch.zeros(rows, 10, 57, device="cuda"), torch.zeros(rows, 29, device="cuda")
    g = torch.Generator().manual_seed(1)
    draw = lambda: (torch.randn(rows, 10, 57, generator=g), torch.randn(rows, 29, generator=g) / rows)

    def step():
        y = he(x)
        fused.assert_recordable_graph([y], "history encoder")
        return torch.autograd.grad(y, params, gy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = step()
    from tests.test_activations import _rows_off_the_kinks
    for session in range(3):
        xs, gs = draw()
        xk = xs * (0.5 + session)
        # rows with a pre-activation inside fp32's resolution of the activation's kink carry no gradient (tests/test_activations.py)
        gs = gs * _rows_off_the_kinks((he64,), lambda: he64(xk.double()), (he32,), lambda: he32(xk), rows, f"history encoder under replay {name} {session}")[:, None]
        x.copy_(xs * (0.5 + session)); gy.copy_(gs)
        graph.replay()
        torch.cuda.synchronize()
        xs = xs * (0.5 + session)
        for m, xx, gg in ((he64, xs.double(), gs.double()), (he32, xs, gs)):
            for p in m.parameters():
                p.grad = None
            m(xx).backward(gg)
        for (n, p64), p32, got in zip(he64.named_parameters(), he32.parameters(), grads):
            r = p64.grad
            scale = float(r.abs().max())
            own = 3.0 * float((p32.grad.double() - r).abs().max())
            err = float((got.double().cpu() - r).abs().max())
            print("MEASURED history encoder under replay", name, session, n, "err=%.3e scale=%.3e three_x_torch_fp32=%.3e" % (err, scale, own))
            assert err <= max(3e-4 * scale, own), (session, n, err, scale, own)
