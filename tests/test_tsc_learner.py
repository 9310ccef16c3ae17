"""Task-level (TSC) learner mirror vs. the reference's own tsc/rsl_rl run on the same protocol
(tests/golden/tsc_learner.npz, made by tools/gen_golden_tsc.py).  CPU: same torch, same generator, same order of draws
=> the sampled hybrid actions are identical and everything downstream is compared tightly.  GPU: the fused paths
(Linear+ELU backward, qa_gae, qa_clip_adam_step) against the CPU mirror on the same stored rollout."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import tsc_protocol as P

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tsc_learner.npz")


def _mine():
    import quadrupedal_agility_amd.tsc.rsl_rl.algorithms as algs
    import quadrupedal_agility_amd.tsc.rsl_rl.modules as mods
    return mods, algs


def test_state_dict_layout_matches_reference_names():
    mods, algs = _mine()
    ac, bbc, est, _ = P.build(mods, algs)
    keys = set(ac.state_dict())
    for k in ("std", "actor.priv_encoder.0.weight", "actor.priv_encoder.2.bias", "actor.history_encoder.encoder.0.weight",
              "actor.history_encoder.conv_layers.0.weight", "actor.history_encoder.conv_layers.2.weight",
              "actor.history_encoder.linear_output.0.weight", "actor.scan_encoder.0.weight", "actor.scan_encoder.4.weight",
              "actor.actor_trunk.0.weight", "actor.actor_trunk.4.weight", "actor.actor_d.weight", "actor.actor_c.weight",
              "critic.0.weight", "critic.6.weight"):
        assert k in keys, k
    assert ac.state_dict()["actor.actor_c.weight"].shape == (18, 128) and ac.state_dict()["actor.actor_trunk.0.weight"].shape == (512, 65 + 32 + 4 + 29)
    assert len(list(ac.parameters())) == 37                       # the golden's probe has one row per tensor
    assert set(bbc.state_dict()) >= {"std", "priv_encoder.0.weight", "history_encoder.encoder.0.weight", "actor_trunk.0.weight",
                                     "actor_head.weight", "critic_trunk.0.weight", "critic_head.weight"}
    assert bbc.state_dict()["actor_trunk.0.weight"].shape == (512, 101)


def test_protocol_matches_reference_golden():
    g = np.load(GOLD)
    out = P.run(*_mine())
    assert set(out) == set(g.files)
    exact = ("rl_actions", "dagger_actions")                       # column 0 (the sampled gait) must be identical
    for k in g.files:
        a, b = np.asarray(out[k], dtype=np.float64), np.asarray(g[k], dtype=np.float64)
        assert a.shape == b.shape, k
        if k in exact:
            assert np.array_equal(a[..., 0], b[..., 0]), k
        tol = 2e-4 if k.startswith("probe") or k.startswith("update") else 2e-5
        np.testing.assert_allclose(a, b, rtol=tol, atol=tol, err_msg=k)
    assert float(out["lr_after_update"]) == float(g["lr_after_update"])
    assert int(out["counter"]) == 2


def test_hybrid_action_layout_and_log_probs():
    mods, algs = _mine()
    ac, *_ = P.build(mods, algs)
    obs = P.det((7, 800), 77)
    torch.manual_seed(0)
    a = ac.act(obs)
    assert a.shape == (7, 19) and set(a[:, 0].tolist()) <= {0.0, 1.0, 2.0}
    lp_d, lp_c = ac.get_actions_log_prob_d(a[:, 0]), ac.get_actions_log_prob_c(a[:, 1:])
    probs = torch.softmax(ac.actor.actor_d(ac.actor(obs, False)), -1)
    np.testing.assert_allclose(lp_d.detach(), torch.log(probs[torch.arange(7), a[:, 0].long()]).detach(), rtol=1e-5, atol=1e-6)
    z = (a[:, 1:] - ac.action_mean) / ac.action_std
    ref = (-0.5 * z * z - torch.log(ac.action_std) - 0.5 * np.log(2 * np.pi)).sum(-1)
    np.testing.assert_allclose(lp_c.detach(), ref.detach(), rtol=1e-5, atol=1e-5)
    inf = ac.act_inference(obs)
    assert torch.equal(inf[:, 0], probs.argmax(-1).float())


def test_depth_heads_are_optional_as_in_the_reference():
    """ppo.py:82-93: depth_encoder None = teacher training only (no student optimisers); the student path is tests/test_tsc_depth.py"""
    mods, algs = _mine()
    ac, bbc, est, _ = P.build(mods, algs)
    alg = algs.PPO(ac, bbc, est, P.ESTIMATOR, None, {}, None)
    assert not alg.if_depth and not hasattr(alg, "depth_actor_optimizer") and alg.update_depth_actor(*[None] * 7) is None


@pytest.mark.gpu
def test_gpu_update_matches_cpu_mirror():
    """Same stored rollout, one minibatch per epoch (so the device's own permutation only reorders a mean)."""
    mods, algs = _mine()
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    assert fused.ENABLED
    res = {}
    for dev in ("cpu", "cuda"):
        ac, bbc, est, _ = P.build(mods, algs)
        cfg = dict(P.ALGO, num_mini_batches=1, num_learning_epochs=2, schedule="fixed")
        alg = algs.PPO(ac, bbc, est, P.ESTIMATOR, None, None, None, device=dev, **cfg)
        est.to(dev)
        alg.init_storage(P.N, P.T, [800], [800], [19])
        torch.manual_seed(5)
        for t in range(P.T):
            o = P.det((P.N, 800), 100 + t).to(dev)
            alg.act(o, o, None)
            if dev == "cuda":                                   # replay the CPU run's sampled actions so the two rollouts coincide
                tr, a = alg.transition, res["cpu"]["actions"][t].to(dev)
                tr.actions = a
                tr.actions_log_prob_d = ac.get_actions_log_prob_d(a[:, 0]).detach()
                tr.actions_log_prob_c = ac.get_actions_log_prob_c(a[:, 1:]).detach()
            else:
                res.setdefault("cpu", {}).setdefault("actions", []).append(alg.transition.actions.clone())
            alg.process_env_step(P.det((P.N,), 200 + t).to(dev), (P.det((P.N,), 300 + t) > 0.8).to(dev), {})
        alg.compute_returns(P.det((P.N, 800), 500).to(dev))
        r = res.setdefault(dev, {})
        r["returns"], r["adv"] = alg.storage.returns.cpu().clone(), alg.storage.advantages.cpu().clone()
        r["update"] = np.asarray(alg.update())
        r["probe"], r["probe_est"] = P.param_probe(ac.cpu()), P.param_probe(est.cpu())
    c, g = res["cpu"], res["cuda"]
    np.testing.assert_allclose(g["returns"], c["returns"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["adv"], c["adv"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(g["update"], c["update"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(g["probe"], c["probe"], rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(g["probe_est"], c["probe_est"], rtol=5e-3, atol=5e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("N,sync_phases", [(1024, False), (1024, True), (8192, False)])
def test_recorded_update_equals_eager_update(N, sync_phases):
    """PPO._update_recorded (the minibatch step as hipGraph replays, LR rule + both Adam steps on the device) against the eager loop on
    the same stored rollouts and the same permutations, over FIVE updates on new data each (update 0 is eager in both -- it creates the
    Adam state --, 1 records, 2-4 are replay sessions), with the host reading nothing between updates and with a device sync after
    every phase (torch's stale batch reductions only showed without syncs and only from the second replay session on:
    profiles/r2_hipgraph_stale_reductions.md).  Both runs issue the same kernels in the same order, so the parameters, the learning
    rate and the loss read-out are held to 1e-6 (8,192 envs: a schedule that follows the amplification, see the assertion) -- not to the 2e-3 of a check that would pass on a frozen bias."""
    mods, algs = _mine()
    res = {}
    for mode in ("eager", "recorded"):
        ac, bbc, est, _ = P.build(mods, algs)
        cfg = dict(P.ALGO, num_mini_batches=4, num_learning_epochs=2, schedule="adaptive", desired_kl=0.01)
        est.to("cuda")
        alg = algs.PPO(ac, bbc, est, P.ESTIMATOR, None, None, None, device="cuda", **cfg)
        alg.use_update_graph = mode == "recorded"
        alg.init_storage(N, P.T, [800], [None], [19])
        snaps = []
        for it in range(5):
            torch.manual_seed(5 + it)
            with torch.inference_mode():
                for t in range(P.T):
                    o = P.det((N, 800), 100 + t + 50 * it).cuda()
                    alg.act(o, o, None)
                    alg.process_env_step(P.det((N,), 200 + t + 7 * it).cuda(), (P.det((N,), 300 + t + 3 * it) > 0.8).cuda(), {})
                alg.compute_returns(P.det((N, 800), 500 + it).cuda())
            if sync_phases:
                torch.cuda.synchronize()
            torch.manual_seed(99 + it)                        # the permutation of this update
            out = alg.update()
            if sync_phases:
                torch.cuda.synchronize()
            # device-side snapshots only: nothing is read back until all five updates have been issued
            snaps.append([p.detach().clone() for p in list(ac.parameters()) + list(est.parameters())] + [torch.as_tensor(np.asarray(out, dtype=np.float64))])
        assert (alg._graph not in (None, False)) == (mode == "recorded")
        res[mode] = dict(snaps=snaps, lr=alg.learning_rate)
    e, r = res["eager"], res["recorded"]
    assert r["lr"] == pytest.approx(e["lr"], rel=1e-6) and e["lr"] != P.ALGO.get("learning_rate", 1e-3)     # the rule moved it, the same way
    for it in range(5):
        moved = 0
        for k, (pe, pr) in enumerate(zip(e["snaps"][it], r["snaps"][it])):
            d = (pe.double().cpu() - pr.double().cpu()).abs().max().item()
            # 1024 envs: both runs launch the same kernels (r6: the chain step, eager and recorded alike) -> 1e-6.
            if N <= 1024:
                assert d <= 1e-6, f"update {it}, tensor {k}: recorded and eager differ by {d}"
                continue
            # 8192 envs (49,152-row steps on the library's GEMMs, whose split of a product can differ between an eager call and a recorded one): the first
            # difference is ~1e-6 after update 1 and grows ~10x per update -- Adam normalises every gradient to O(learning rate), the adaptive rate follows,
            # and a tensor like the 18 log-stds (one sum over all rows each) differs in EVERY element.  How fast depends on the box, not on the run (four
            # runs on one box gave the same digits); on five r6 boxes: <= 1.1e-6 after update 1, 1.1e-6 .. 4.2e-5 after update 2, <= 3.3e-4 after update 3.
            # What the test guards -- a stale reduction under replay, the r2 finding -- freezes or corrupts a whole tensor: 8e-3 per recorded update (8 steps
            # at 1e-3), i.e. 8e-3 x `it` by update `it`, NaN / inf at worst; the schedule 1e-5, 1e-4, 1e-3, 1e-2 stays under that, and the "every tensor
            # moved" check below sees a frozen one directly
            bound = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2)[it]
            assert d <= bound, f"update {it}, tensor {k}: recorded and eager differ by {d} (bound {bound})"
        if it:           # every tensor these steps train moved (the history encoder is the DAgger step's: 8 tensors stay) -- no frozen gradient
            moved = sum(int(not torch.equal(a, b)) for a, b in zip(r["snaps"][it][:-1], r["snaps"][it - 1][:-1]))
            assert moved == len(r["snaps"][it]) - 1 - 8, f"update {it}: {moved} tensors moved"


@pytest.mark.gpu
def test_recorded_dagger_update_equals_eager_dagger_update():
    """PPO.update_dagger (the history-encoder regression of every 20th iteration) as replays of one recorded step against the eager loop: the same
    stored rollouts, the same permutations, four updates (0 eager in both, 1 records, 2-3 replay sessions)."""
    mods, algs = _mine()
    res = {}
    N = 1024
    for mode in ("eager", "recorded"):
        ac, bbc, est, _ = P.build(mods, algs)
        est.to("cuda")
        alg = algs.PPO(ac, bbc, est, P.ESTIMATOR, None, None, None, device="cuda", **dict(P.ALGO, num_mini_batches=4, num_learning_epochs=2))
        alg.init_storage(N, P.T, [800], [None], [19])
        if mode == "eager":
            alg._dagger_graph = False
        hp = list(ac.actor.history_encoder.parameters())
        snaps = []
        for it in range(4):
            torch.manual_seed(5 + it)
            with torch.inference_mode():
                for t in range(P.T):
                    o = P.det((N, 800), 100 + t + 50 * it).cuda()
                    alg.act(o, o, None)
                    alg.process_env_step(P.det((N,), 200 + t + 7 * it).cuda(), (P.det((N,), 300 + t + 3 * it) > 0.8).cuda(), {})
            torch.manual_seed(99 + it)
            loss = alg.update_dagger()
            snaps.append(([p.detach().clone() for p in hp], loss))
        assert (alg.__dict__.get("_dagger_graph") not in (None, False)) == (mode == "recorded")
        res[mode] = snaps
    for it, ((pe, le), (pr, lr_)) in enumerate(zip(res["eager"], res["recorded"])):
        assert lr_ == pytest.approx(le, rel=1e-5), (it, le, lr_)
        for k, (a, b) in enumerate(zip(pe, pr)):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (it, k, float((a - b).abs().max()))
        if it:
            assert all(not torch.equal(a, b) for a, b in zip(pr, res["recorded"][it - 1][0]))       # every tensor of the encoder moved


@pytest.mark.gpu
def test_networks_outside_the_whitelist_stay_eager():
    """fused.recordable: a recorded step may only contain gradients our kernels produce (the task-level update used to be
    recorded whatever the networks were; a wide scan-encoder output or another activation put torch's bias reductions into the graph)"""
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    mods, algs = _mine()
    ac, bbc, est, _ = P.build(mods, algs)
    assert fused.recordable(ac, est)
    ac.actor.scan_encoder[0].bias = None                       # a Linear without a bias falls back to F.linear
    assert not fused.recordable(ac, est)
    ac2, _, est2, _ = P.build(mods, algs)
    ac2.extra = torch.nn.GRU(4, 4)                             # a module whose gradients are not ours
    assert not fused.recordable(ac2, est2)
    # a plain Linear wider than the narrow-head kernel (scan latent of 48) is still ours: one-layer _MlpChain, no torch reduction
    lin = torch.nn.Linear(64, 48).cuda()
    x = torch.randn(300, 64, device="cuda", requires_grad=True)
    y = fused.plain_linear(lin, x)
    assert y.grad_fn is not None and "MlpChain" in type(y.grad_fn).__name__
    y.backward(torch.ones_like(y))
    ref = torch.nn.functional.linear(x.detach(), lin.weight.detach(), lin.bias.detach())
    assert torch.allclose(y.detach(), ref, rtol=1e-5, atol=1e-5) and torch.allclose(lin.bias.grad, torch.full((48,), 300.0, device="cuda"))


def test_rollout_keeps_the_observation_the_action_was_drawn_from():
    """the env overwrites its observation buffer in place during step(): the row stored for step t must be the one act() saw, not
    what the buffer holds when process_env_step() runs (regression: the rows used to be copied there, one step late)"""
    mods, algs = _mine()
    ac, bbc, est, _ = P.build(mods, algs)
    alg = algs.PPO(ac, bbc, est, P.ESTIMATOR, None, None, None, device="cpu", **P.ALGO)
    alg.init_storage(P.N, P.T, [800], [None], [19])
    buf = P.det((P.N, 800), 1).clone()
    seen = []
    for t in range(3):
        seen.append(buf.clone())
        alg.act(buf, buf, None)
        buf.copy_(P.det((P.N, 800), 2 + t))                 # "env.step" rewrites the same tensor
        alg.process_env_step(P.det((P.N,), 200 + t), P.det((P.N,), 300 + t) > 0.8, {})
    for t in range(3):
        assert torch.equal(alg.storage.observations[t], seen[t])


@pytest.mark.gpu
def test_hybrid_ppo_loss_kernel_matches_its_c_twin():
    """qa_hybrid_ppo_loss vs qo_hybrid_ppo_loss (itself checked against torch's eager objective + autograd on CPU,
    tests/test_learner_twins_cpu.py): loss terms and the four gradients, incl. a batch that is not a multiple of the block"""
    import ctypes as C
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    from tests.oracle_lib import load_oracle
    f = load_oracle().qo_hybrid_ppo_loss
    for B in (1000, 49152):
        torch.manual_seed(B)
        ND, NC = 3, 18
        logits, mean, std, value = torch.randn(B, ND) * 2, torch.randn(B, NC), torch.rand(NC) * 0.8 + 0.3, torch.randn(B)
        a_d = torch.randint(0, ND, (B,))
        actions = torch.cat([a_d.float().unsqueeze(1), mean + torch.randn(B, NC) * 0.7], 1)
        old_mu, old_sigma = mean + 0.1 * torch.randn(B, NC), (std * 1.05).expand(B, NC).contiguous()
        old_logp_d = torch.log_softmax(logits + 0.3 * torch.randn(B, ND), -1)[torch.arange(B), a_d]
        old_logp_c = torch.distributions.Normal(old_mu, old_sigma).log_prob(actions[:, 1:]).sum(-1) + 0.2 * torch.randn(B)
        adv, ret, tv = torch.randn(B), torch.randn(B), value + 0.3 * torch.randn(B)
        ins = [x.contiguous() for x in (logits, mean, std, value, actions, old_logp_d, old_logp_c, old_mu, old_sigma, adv, ret, tv)]
        dlg, dmu, dsd, dv, out = torch.empty(B, ND), torch.empty(B, NC), torch.empty(NC), torch.empty(B), torch.empty(8)
        assert f(*[t.data_ptr() for t in ins], B, ND, NC, 0.2, 1.0, 0.01, 1, dlg.data_ptr(), dmu.data_ptr(), dsd.data_ptr(), dv.data_ptr(), out.data_ptr(), None, 0, None) == 0
        g = [t.cuda() for t in ins]
        o, gl, gm, gs, gv = fused.hybrid_ppo_loss_raw(*g, clip=0.2, c_value=1.0, c_entropy=0.01, clipped_value=True)
        assert np.allclose(o.cpu().numpy()[:7], out.numpy()[:7], rtol=3e-5, atol=3e-6)
        for got, want in ((gl, dlg), (gm, dmu), (gs, dsd), (gv, dv)):
            assert torch.allclose(got.cpu(), want, rtol=3e-4, atol=1e-7 + 3e-4 / B)


def _hybrid_case(n=4096, nd=6, nc=18, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, nd, generator=g) * 1.5
    logits[:64, 0] += 40.0                                   # near-deterministic rows: the eps clamp of Categorical(probs) matters
    mean = torch.randn(n, nc, generator=g)
    std = torch.rand(nc, generator=g) * 0.8 + 0.2
    value = torch.randn(n, generator=g)
    hist = torch.randn(n, 8, 1 + nc, generator=g)
    return logits, mean, std, value, hist


def _run_hybrid(lib, prefix, t, step, dev=None, out_of_place=False):
    logits, mean, std, value, hist = (x.clone().to(dev) if dev else x.clone() for x in t)
    hist_in = None
    if out_of_place:
        hist_in, hist = hist, torch.zeros_like(hist)
    n, nd = logits.shape; nc = mean.shape[1]
    z = lambda *s: torch.zeros(*s, device=dev) if dev else torch.zeros(*s)
    out = dict(actions=z(n, 1 + nc), st_actions=z(n, 1 + nc), mu=z(n, nc), sigma=z(n, nc), logp_d=z(n), logp_c=z(n), values=z(n), hist=hist)
    ctr = torch.tensor([step], dtype=torch.int64, device=dev) if dev else torch.tensor([step], dtype=torch.int64)
    P = lambda x: x.data_ptr()
    rc = getattr(lib, prefix + "rollout_act_hybrid")(P(logits), P(mean), P(std), P(value), 12345, P(ctr), 0, n, 100, nd, nc, P(out["actions"]), P(out["st_actions"]), P(out["mu"]),
                                                      P(out["sigma"]), P(out["logp_d"]), P(out["logp_c"]), P(out["values"]), P(hist_in) if hist_in is not None else None, P(hist), 8, None)
    assert rc == 0
    return out


def test_hybrid_act_twin_matches_torch_distributions():
    """qa_rollout_act_hybrid's C twin: the log-probabilities are torch's Categorical(probs=softmax(logits)) / Normal log_prob of the sampled action,
    the choice follows the softmax probabilities (chi-square over 4096 x 8 draws), the Gaussian part has the right moments, storage rows and the
    action-history roll are what PPO.act / add_transitions / the runner wrote with ten-odd torch ops"""
    from torch.distributions import Categorical, Normal
    from tests.oracle_lib import load_oracle
    lib = load_oracle()
    t = _hybrid_case()
    logits, mean, std, value, hist = t
    counts = torch.zeros(6)
    for step in range(8):
        o = _run_hybrid(lib, "qo_", t, step)
        a_d, a_c = o["actions"][:, 0].long(), o["actions"][:, 1:]
        assert torch.equal(o["actions"], o["st_actions"]) and torch.equal(o["mu"], mean) and torch.equal(o["sigma"], std.expand_as(mean)) and torch.equal(o["values"], value)
        dist_d = Categorical(probs=torch.softmax(logits, -1), validate_args=False)
        assert torch.allclose(o["logp_d"], dist_d.log_prob(a_d), rtol=1e-5, atol=2e-6)
        assert torch.allclose(o["logp_c"], Normal(mean, std.expand_as(mean)).log_prob(a_c).sum(-1), rtol=1e-5, atol=2e-5)
        assert torch.equal(o["hist"][:, :-1], hist[:, 1:]) and torch.equal(o["hist"][:, -1], o["actions"])
        counts += torch.bincount(a_d[64:], minlength=6).float()
        z = (a_c - mean) / std
        assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
        assert (a_d[:64] == 0).all()
    expect = torch.softmax(logits[64:], -1).sum(0) * 8
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 25.0, chi2                                  # 5 degrees of freedom: p < 1e-4 beyond 25
    o2 = _run_hybrid(lib, "qo_", t, 3)
    assert torch.equal(o2["actions"], _run_hybrid(lib, "qo_", t, 3)["actions"]) and not torch.equal(o2["actions"], o["actions"])     # keyed by the step


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5000, 8192])      # a single env, a ragged last workgroup, BASELINE configs[3]'s env count
def test_hybrid_act_kernel_matches_twin(n):
    from quadrupedal_agility_amd import _capi
    from tests.oracle_lib import load_oracle
    t = _hybrid_case(n=n, seed=2)
    for step in (0, 7):
        a = _run_hybrid(_capi.load_library(), "qa_", t, step, dev="cuda")
        a2 = _run_hybrid(_capi.load_library(), "qa_", t, step, dev="cuda", out_of_place=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a[k], a2[k]) for k in a)          # in-place and out-of-place history rolls agree
        b = _run_hybrid(load_oracle(), "qo_", t, step)
        b2 = _run_hybrid(load_oracle(), "qo_", t, step, out_of_place=True)
        assert all(torch.equal(b[k], b2[k]) for k in b)
        same = a["actions"][:, 0].cpu() == b["actions"][:, 0]
        assert same.float().mean() > (0.999 if n > 1 else 0.5)      # a uniform within rounding of a CDF edge may fall on the other side (expf ulps)
        for k in ("actions", "st_actions", "mu", "sigma", "logp_d", "logp_c", "values", "hist"):
            x, y = a[k].cpu(), b[k]
            m = same if x.dim() == 1 else same.view(-1, *([1] * (x.dim() - 1))).expand_as(x)
            assert torch.allclose(x[m], y[m], rtol=2e-5, atol=2e-5), k
